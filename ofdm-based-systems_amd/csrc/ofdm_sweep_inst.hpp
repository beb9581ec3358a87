// ofdm_sweep_inst.hpp -- launcher of the one-pass SNR sweep receiver (ofdm_rx_sweep); included once
// per precision by ofdm_kernels_f32_sweep.hip / ofdm_kernels_f64_sweep.hip, translation units of their
// own beside the k_rx and k_rx_prof ones (parallel compile, and every other object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing: the complex128 cyclic-prefix OFDM fixed-QAM bench shapes -- 64-QAM at N = 1024, 256-QAM at
// N = 4096 -- take their throughput receiver's k_rx_sweep, by equaliser.  Everything else takes the
// generic kernel's: complex64, SC-OFDM, zero padding, PSK, N < 64, adaptive plans (one plan for every
// point: adaptive loading re-derived per SNR is a different plan per point and not a sweep).
template <int LOGN>
constexpr int sweep_fb() { return LOGN == 10 ? 6 : LOGN == 12 ? 8 : 0; }

template <typename R, int LOGN, int EQ, int FB>
static hipError_t rx_sweep_launch(const RxSweepArgs& a, int* grid, hipStream_t s) {
    constexpr bool MV = FB == 0;  // (the generic kernel as rx_one launches it; compiled out of the fixed-QAM ones)
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, true>();
    using G = Geo<LOGN, BLK>;
    const TxRxCommon& c = a.r.c;
    CarveSize lds;
    rx_carve<R, LOGN, EQ, FB, MV, true>(lds, c.words_per_sym, rx_tts<R, LOGN, FB>(FB == 0 && c.scm), 0, a.n_snr);
    const size_t sm = lds.bytes;
    if (sm + rx_static_lds<R, FB>() > kLdsPerCu) {
        // (a layout that does not fit: the generic kernel, which is the last resort)
        if constexpr (FB > 0)
            return rx_sweep_launch<R, LOGN, -1, 0>(a, grid, s);
        else
            return kLdsOverflow;
    }
    auto fn = k_rx_sweep<R, LOGN, EQ, FB, MV>;
    hipError_t e = set_smem(fn, sm);
    if (e != hipSuccess) return e;
    // Every workgroup builds a table per point and ends with an atomic pair per point: two rounds of
    // the resident workgroups, each looping over its share of the symbols (as the profile's launcher)
    const int64_t want = (c.n_sym + G::SPB - 1) / G::SPB;
    const int res = resident_blocks(fn, BLK, sm);
    *grid = clamp_grid(res > 0 ? std::min<int64_t>(want, 2 * (int64_t)res) : want);
    hipLaunchKernelGGL(fn, dim3(*grid), dim3(BLK), sm, s, a);
    return hipGetLastError();
}

template <typename R, int LOGN>
static hipError_t rx_sweep_one(const RxSweepArgs& a, int* grid, hipStream_t s) {
    if constexpr (sizeof(R) == 8 && sweep_fb<LOGN>() > 0) {
        constexpr int FB = sweep_fb<LOGN>();
        const TxRxCommon& c = a.r.c;
        if (fixed_fast(c) && c.psk_m == 0 && c.b == FB && !c.scm && !c.zpad) {
            if (c.eq == OFDM_EQ_NONE) return rx_sweep_launch<R, LOGN, OFDM_EQ_NONE, FB>(a, grid, s);
            if (c.eq == OFDM_EQ_ZF) return rx_sweep_launch<R, LOGN, OFDM_EQ_ZF, FB>(a, grid, s);
            return rx_sweep_launch<R, LOGN, OFDM_EQ_MMSE, FB>(a, grid, s);
        }
    }
    return rx_sweep_launch<R, LOGN, -1, 0>(a, grid, s);
}

template <typename R>
hipError_t launch_rx_sweep(int logn, const RxSweepArgs& a, int* grid, hipStream_t s) {
    if (a.n_snr < 1 || a.n_snr > OFDM_MAX_SWEEP_POINTS || a.r.wide != nullptr) return hipErrorInvalidValue;
#define OFDM_RX_SWEEP_CASE(L) \
    case L:                   \
        return rx_sweep_one<R, L>(a, grid, s);
    switch (logn) {
        OFDM_LOGN_CASES(OFDM_RX_SWEEP_CASE)
        default:
            return kOutOfRange;
    }
#undef OFDM_RX_SWEEP_CASE
}

#define OFDM_INSTANTIATE_RX_SWEEP(R) \
    template hipError_t launch_rx_sweep<R>(int, const RxSweepArgs&, int*, hipStream_t);

}  // namespace ofdm
