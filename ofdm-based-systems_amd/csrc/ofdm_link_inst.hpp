// ofdm_link_inst.hpp -- the fused link kernel k_link (ofdm_link) and its launcher; included by
// ofdm_kernels_f64_link.hip, a translation unit of its own beside the k_tx / k_rx / k_rx_prof /
// k_rx_sweep ones (every other object stays as it was).
//
// k_link transmits and receives a symbol in one wave without the kept channel samples y leaving the
// registers: the flat transmitter's sequence (lane block -> LUT gather -> IFFT: the statements of
// k_tx<double, LOGN, FB, 0> on the same templates, in the same order, so the registers hold the values
// k_tx would have stored) and then the no-equaliser receiver's body on them in place of its buffer
// loads (add_noise64 -> FFT -> slicer -> XOR / popcount -> the u64 atomics: ofdm_rx_body.hpp's
// statements for F64_FAST, EQ = NONE, MV = false).  The lane's Philox block is drawn once and serves
// both halves.  No y store, no y load, no statistics: the power the noise is scaled by, sum |x|^2 and
// the peak come from the power pass (ofdm_tx with y = NULL) over the whole stream.
//
// Shape: complex128, fixed square QAM of FB bits, cyclic-prefix OFDM (or no prefix), flat channel,
// Philox streams, no equaliser -- bench config (b) at N = 1024, FB = 6.
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// The workgroup: both transforms' per-pass twiddles (the inverse ones are the forward ones' exact
// conjugates, held as the plan uploads them: [forward | inverse]) and the LUT beside the rows leave
// room for 12 symbols' rows of reals, not the receiver's 16 -- 768 threads, 3 waves per SIMD
// (168 VGPRs: nothing spilled, where the 1024-thread receiver spills 6 dwords at 128).
#ifndef OFDM_LINK_BLOCK
#define OFDM_LINK_BLOCK 768
#endif
#ifndef OFDM_LINK_WAVES
#define OFDM_LINK_WAVES 3
#endif

template <typename R>
struct LinkLds {
    cpx<R>* tt;  // per-pass twiddles [forward | inverse]
    AxisInfo* axis;
    unsigned char* rowmem;
    unsigned long long* redc;
};
template <typename R, int LOGN, typename CV>
__host__ __device__ __forceinline__ constexpr LinkLds<R> link_carve(CV& cv) {
    using G = Geo<LOGN, OFDM_LINK_BLOCK>;
    LinkLds<R> m{};
    m.axis = cv.template take<AxisInfo>(kMaxLuts);
    m.rowmem = cv.template take<unsigned char>((size_t)G::SPB * G::PADN * sizeof(R));
    m.redc = cv.template take<unsigned long long>(OFDM_LINK_BLOCK / 64);
    m.tt = cv.template take<cpx<R>>(2 * tt_size(LOGN));
    return m;
}
// static LDS: the transmitter's LUT, the noise phase table and its widening to double
template <typename R, int FB>
constexpr size_t link_static_lds() { return (1 << FB) * sizeof(cpx<R>) + rx_static_lds<R, FB>(); }

template <typename R, int LOGN, int FB>
__global__ __launch_bounds__(OFDM_LINK_BLOCK, OFDM_LINK_WAVES) void k_link(LinkArgs la) {
    static_assert(sizeof(R) == 8 && FB > 1 && !(FB & 1), "complex128 fixed square QAM");
    static_assert(uses_tt<R, LOGN, FB>() && Geo<LOGN>::TPS >= 64, "a symbol per wave, per-pass twiddles in LDS");
    constexpr int BLK = OFDM_LINK_BLOCK;
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr int E = G::E, TPS = G::TPS;
    constexpr int TTS = tt_size(LOGN);
    const RxArgs& a = la.r;
    const TxRxCommon& cm = a.c;
    __shared__ C lut_s[1 << FB];
    __shared__ f32x2 ntab[kNoisePhases];
    __shared__ f64x2 ntab64[kNoisePhases];
    Carve cv(ofdm_smem);
    const LinkLds<R> lds = link_carve<R, LOGN>(cv);
    C* tt = lds.tt;
    AxisInfo* axis = lds.axis;
    unsigned long long* redc = lds.redc;

    // the tables' global reads issued first (Staged), the noise table built while they fly
    Staged<BLK, 2 * TTS, C> st_tt;
    Staged<BLK, (1 << FB), C, true> st_lut;
    Staged<BLK, kMaxLuts, Dwords<AxisInfo>> st_ax;
    static_assert(kMaxLuts <= BLK, "one axis entry per thread");
    const C hf = ((const C*)la.h)[0];
    st_tt.load((const C*)cm.ptw, 2 * TTS);
    st_lut.load((const C*)cm.lut, cm.lut_len);
    st_ax.load((const Dwords<AxisInfo>*)cm.axis, cm.n_axis);
    // sigma from the whole-stream mean power (as k_rx)
    const bool noise = a.noise_on;
    double sigma_d = 0;
    if (noise) {
        const double p = a.stats[0] / (double)a.total_samples;
        sigma_d = sqrt((p / a.snr_lin) / 2.0);
    }
    build_noise_table(ntab, sigma_d, ntab64);
    st_tt.store(tt);
    // the 1/sqrt(N) of ifft(norm="ortho") and the channel tap folded into the LUT (as k_tx, FOLD_H0)
    const R lut_scale = (R)cm.scale;
    st_lut.store(lut_s, [&](const C& v) { return cscale(cmul(hf, v), lut_scale); });
    st_ax.store((Dwords<AxisInfo>*)axis);
    __syncthreads();

    const int ls = __builtin_amdgcn_readfirstlane(threadIdx.x / TPS);
    const int t = threadIdx.x % TPS;
    C* row = (C*)(lds.rowmem + (size_t)ls * G::PADN * sizeof(R));
    PermSlicer64<FB> pslicer;
    pslicer.load(axis[0], cm.scale);  // the FFT output stays unscaled (x sqrt N)

    const int64_t niter = (cm.n_sym + G::SPB - 1) / G::SPB;
    unsigned long long be = 0, se = 0;
    for (int64_t it = blockIdx.x; it < niter; it += gridDim.x) {
        const int64_t sl = it * G::SPB + ls;
        const int64_t sg = cm.sym0 + sl;
        const bool active = sl < cm.n_sym;
        // the lane block: bits for both halves, the generator continuing into the lane's noise
        TxBits<FB, TPS> tb;
        tb.load(cm, sg, t, nullptr, active);
        // transmitter: map and IFFT; x leaves the IFFT as the channel output y
        C x[E];
        static_for<0, E>([&](auto I) { x[I] = lut_s[tb.template fixed<I>()]; });
        fft_sym<R, LOGN, true, FB>(x, row, tt, tt + TTS, t);
        sym_sync<TPS>();  // the IFFT's last pass has read the row
        // receiver: y + AWGN, FFT, slice, compare, count
        if (active && noise) {
#pragma unroll
            for (int i = 0; i < E; ++i) tb.g.add_noise64(x[i].re, x[i].im, ntab64, i);
        }
        fft_sym<R, LOGN, false, FB>(x, row, tt, tt, t);
        if (active) {
            uint32_t bes = 0, ses = 0;
            static_for<0, E / 4>([&](auto Q) {
                constexpr int q = Q;
                C z[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) z[j] = x[4 * q + j];
                const uint32_t d = pslicer.diff(z, lane_word(tb.lane, q));
                bes += __popc(d);
                ses += PermSlicer<FB>::nonzero_bytes(d);
            });
            be += bes;
            se += ses;
        }
        sym_sync<TPS>();  // the FFT row is rewritten by the next symbol
    }
    be = block_sum<unsigned long long, BLK>(be, redc);
    se = block_sum<unsigned long long, BLK>(se, redc);
    if (threadIdx.x == 0) {
        if (be) atomicAdd((unsigned long long*)&a.counters[0], be);
        if (se) atomicAdd((unsigned long long*)&a.counters[1], se);
    }
}

// What has a fused form (the one definition: launch_link answers hipErrorInvalidValue for anything
// else and ofdm_link names the reason): a complex128 fixed-QAM bench shape (ref_fb > 1) at a symbol per
// wave with its per-pass twiddles in LDS, a flat channel, no equaliser, Philox streams.
template <typename R, int LOGN>
constexpr int link_fb() {
    if constexpr (sizeof(R) == 8 && ref_fb<R, LOGN>() > 1 && Geo<LOGN>::TPS == 64) {
        if (uses_tt<R, LOGN, ref_fb<R, LOGN>()>()) return ref_fb<R, LOGN>();
    }
    return 0;
}
template <typename R, int LOGN>
static bool link_shape(const LinkArgs& a, int L) {
    if constexpr (link_fb<R, LOGN>() == 0) return false;
    else
        return bench_fixed_shape<link_fb<R, LOGN>()>(a.r.c) && L == 1 && a.r.c.eq == OFDM_EQ_NONE &&
               philox_streams(a.r) && a.r.wide == nullptr;
}

template <typename R, int LOGN>
static hipError_t link_one(const LinkArgs& a, int L, int* grid, hipStream_t s) {
    if constexpr (link_fb<R, LOGN>() > 0) {
        if (!link_shape<R, LOGN>(a, L)) return hipErrorInvalidValue;
        constexpr int FB = link_fb<R, LOGN>();
        constexpr int BLK = OFDM_LINK_BLOCK;
        CarveSize lds;
        link_carve<R, LOGN>(lds);
        static_assert(Geo<LOGN, BLK>::SPB * Geo<LOGN, BLK>::TPS == BLK, "whole symbols per workgroup");
        if (lds.bytes + link_static_lds<R, FB>() > kLdsPerCu) return kLdsOverflow;
        // one workgroup holds a CU: two rounds of the resident workgroups, as the receiver it replaces
        return rx_go<BLK, Geo<LOGN, BLK>::SPB>(k_link<R, LOGN, FB>, lds.bytes, rx_grid_rounds<R, FB, LOGN>(),
                                               a.r.c.n_sym, a, grid, s);
    } else {
        return hipErrorInvalidValue;
    }
}

// hipErrorInvalidValue: no fused form for this plan or these arguments (nothing launched)
template <typename R>
hipError_t launch_link(int logn, int L, const LinkArgs& a, int* grid, hipStream_t s) {
#define OFDM_LINK_CASE(LG) \
    case LG:               \
        return link_one<R, LG>(a, L, grid, s);
    switch (logn) {
        OFDM_LOGN_CASES(OFDM_LINK_CASE)
        default:
            return kOutOfRange;
    }
#undef OFDM_LINK_CASE
}

}  // namespace ofdm
