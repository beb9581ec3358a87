// ofdm_prof_inst.hpp -- launcher of the receiver with the per-subcarrier profile (ofdm_rx_profile);
// included once per precision by ofdm_kernels_f32_prof.hip / ofdm_kernels_f64_prof.hip, translation
// units of their own beside the k_rx ones (parallel compile, and every k_rx object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing with a profile: the bench shapes -- complex128 cyclic-prefix OFDM, 64-QAM at N = 1024,
// adaptive square-QAM loading at N = 2048, 256-QAM at N = 4096: the shapes ref_fb names -- with Philox
// streams (no caller bits or normals) and no received-symbol tap take their throughput receiver's
// k_rx_prof.  Everything else takes the generic kernel's: caller bits, caller normals or a tap (the
// bench shapes included), complex64, every other shape; a plan with an order above 256 its WIDE form.
// The REF instantiations have no profile.
template <typename R, int LOGN, bool WIDE>
static hipError_t rx_prof_launch(const RxArgs& a, int* grid, hipStream_t s) {
    constexpr int BLK = rx_block<R, 0, LOGN, -1, true>();
    using G = Geo<LOGN, BLK>;
    CarveSize lds;
    rx_carve<R, LOGN, -1, 0, true>(lds, a.c.words_per_sym, rx_tts<R, LOGN, 0>(a.c.scm), WIDE ? a.c.n_axis : 0);
    const size_t sm = lds.bytes;
    // (the profile's symbol slots reuse the FFT rows: no LDS beyond the generic kernel's)
    if (sm + rx_static_lds<R, 0>() > kLdsPerCu) return kLdsOverflow;
    auto fn = k_rx_prof<R, LOGN, -1, 0, true, false, WIDE>;
    hipError_t e = set_smem(fn, sm);
    if (e != hipSuccess) return e;
    // Every workgroup ends with up to five atomics per subcarrier, so the grid is two rounds of the
    // resident workgroups, each looping over its share of the symbols, instead of up to kMaxGrid
    const int64_t want = (a.c.n_sym + G::SPB - 1) / G::SPB;
    const int res = resident_blocks(fn, BLK, sm);
    *grid = clamp_grid(res > 0 ? std::min<int64_t>(want, 2 * (int64_t)res) : want);
    hipLaunchKernelGGL(fn, dim3(*grid), dim3(BLK), sm, s, a);
    return hipGetLastError();
}

template <typename R, int LOGN, int EQ, int FB>
static hipError_t rx_prof_fast(const RxArgs& a, int* grid, hipStream_t s) {
    constexpr bool MV = FB == 1;  // (as rx_one: compiled out of the fixed-QAM kernels; FB = 1 switches it off)
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, true>();
    using G = Geo<LOGN, BLK>;
    CarveSize lds;
    rx_carve<R, LOGN, EQ, FB, MV, true>(lds, a.c.words_per_sym, rx_tts<R, LOGN, FB>(false));
    const size_t sm = lds.bytes;
    // (a layout that does not fit: the generic kernel, as the throughput receivers without a profile)
    if (sm + rx_static_lds<R, FB>() + prof_lut_static<FB>() * sizeof(cpx<R>) > kLdsPerCu)
        return rx_prof_launch<R, LOGN, false>(a, grid, s);
    auto fn = k_rx_prof<R, LOGN, EQ, FB, MV>;
    hipError_t e = set_smem(fn, sm);
    if (e != hipSuccess) return e;
    const int64_t want = (a.c.n_sym + G::SPB - 1) / G::SPB;
    const int res = resident_blocks(fn, BLK, sm);
    *grid = clamp_grid(res > 0 ? std::min<int64_t>(want, 2 * (int64_t)res) : want);
    hipLaunchKernelGGL(fn, dim3(*grid), dim3(BLK), sm, s, a);
    return hipGetLastError();
}

template <typename R, int LOGN>
static hipError_t rx_prof_one(const RxArgs& a, int* grid, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        constexpr int FB = ref_fb<R, LOGN>();
        const TxRxCommon& c = a.c;
        const bool streams = c.bits == nullptr && a.nr == nullptr && a.z_out == nullptr && a.wide == nullptr;
        const bool shape = FB == 1 ? adaptive_fast(c)
                                   : (fixed_fast(c) && c.psk_m == 0 && c.b == FB && !c.scm && !c.zpad);
        if (streams && shape) {
            if (c.eq == OFDM_EQ_NONE) return rx_prof_fast<R, LOGN, OFDM_EQ_NONE, FB>(a, grid, s);
            if (c.eq == OFDM_EQ_ZF) return rx_prof_fast<R, LOGN, OFDM_EQ_ZF, FB>(a, grid, s);
            return rx_prof_fast<R, LOGN, OFDM_EQ_MMSE, FB>(a, grid, s);
        }
    }
    if (a.wide != nullptr) return rx_prof_launch<R, LOGN, true>(a, grid, s);
    return rx_prof_launch<R, LOGN, false>(a, grid, s);
}

template <typename R>
hipError_t launch_rx_prof(int logn, const RxArgs& a, int* grid, hipStream_t s) {
    if (a.profile == nullptr) return hipErrorInvalidValue;
#define OFDM_RX_PROF_CASE(L) \
    case L:                  \
        return rx_prof_one<R, L>(a, grid, s);
    switch (logn) {
        OFDM_LOGN_CASES(OFDM_RX_PROF_CASE)
        default:
            return kOutOfRange;
    }
#undef OFDM_RX_PROF_CASE
}

#define OFDM_INSTANTIATE_RX_PROF(R) template hipError_t launch_rx_prof<R>(int, const RxArgs&, int*, hipStream_t);

}  // namespace ofdm
