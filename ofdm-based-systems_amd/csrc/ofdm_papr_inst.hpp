// ofdm_papr_inst.hpp -- the per-symbol PAPR histogram kernel k_papr (ofdm_papr), its launcher and the
// routing predicate beside it; included once per precision by ofdm_kernels_f32_papr.hip /
// ofdm_kernels_f64_papr.hip, translation units of their own beside the k_tx / k_rx / k_rx_prof /
// k_rx_sweep / k_link ones (every other object stays as it was).
//
// k_papr is the transmitter without a channel, a store or a stream statistic: the lane block, the LUT
// gather and the IFFT are the statements of k_tx on the same templates (throughput form: those of
// k_tx<double, LOGN, FB, 0>, as k_link builds its transmitter half, the LUT scaled by 1 / sqrt N only;
// generic form: those of k_tx<R, LOGN, 0, -1>), then |x|^2 per element, the lane's sum and maximum
// with its share of the prefix by k_tx's prefix_sum rule, both reduced over the symbol's lanes, and
// one lane per symbol bins the pair (ofdm_hip.h: the definition) into the workgroup's histogram in LDS.
// Integer atomics only; the workgroup's non-empty bins leave through one 64-bit atomicAdd each.
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Throughput form: the flat complex128 transmitter's workgroup (1024 threads, 4 waves per SIMD: a
// 128-register budget, which the map, the radix-16 butterfly and the two partials fit unspilled --
// profiles/papr_kernel_audit.txt).  Generic form: the generic transmitter's (256 threads).
#ifndef OFDM_PAPR_BLOCK
#define OFDM_PAPR_BLOCK 1024
#endif
#ifndef OFDM_PAPR_WAVES
#define OFDM_PAPR_WAVES 4
#endif
template <int FB>
constexpr int papr_block() { return FB > 0 ? OFDM_PAPR_BLOCK : kBlock; }
template <int FB>
constexpr int papr_waves() { return FB > 0 ? OFDM_PAPR_WAVES : OFDM_TX_WAVES; }

template <typename R>
struct PaprLds {
    cpx<R> *tw, *lut, *tt;
    AxisInfo* axis;
    unsigned char* rowmem;
    uint32_t* words;
    double* edges;
    uint32_t* hist;
};
// The dynamic LDS of k_papr for the plan's LUT length and staged bit words per symbol (generic form;
// the throughput form's LUT is static LDS): the kernel's layout and the launcher's byte count
template <typename R, int LOGN, int FB, typename CV>
__host__ __device__ __forceinline__ constexpr PaprLds<R> papr_carve(CV& cv, int lut_len, int words_per_sym) {
    using G = Geo<LOGN, papr_block<FB>()>;
    using C = cpx<R>;
    constexpr bool TT = uses_tt<R, LOGN, FB>();
    PaprLds<R> m{};
    m.tw = cv.template take<C>(TT ? 0 : 128);  // two-level twiddles (generic form)
    m.lut = cv.template take<C>(FB == 0 ? lut_len : 0);
    m.axis = cv.template take<AxisInfo>(kMaxLuts);
    // a symbol's FFT row (throughput form: of reals, fft_reg_split); N >= 2048: its first reals
    // carry the symbol's per-wave partials after the transform
    m.rowmem = cv.template take<unsigned char>((size_t)G::SPB * G::PADN * (split_rows<R, FB>() ? sizeof(R) : sizeof(C)));
    m.words = cv.template take<uint32_t>(FB ? 0 : (size_t)G::SPB * words_per_sym);  // reference bits
    m.tt = cv.template take<C>(TT ? tt_size(LOGN) : 0);  // throughput form: inverse per-pass twiddles
    m.edges = cv.template take<double>(OFDM_MAX_PAPR_EDGES);
    m.hist = cv.template take<uint32_t>(OFDM_MAX_PAPR_EDGES + 1);
    return m;
}
template <typename R, int FB>
constexpr size_t papr_static_lds() { return (FB > 1 ? (size_t)1 << FB : 1) * sizeof(cpx<R>); }

// Sum and maximum over the TPS lanes of one symbol (t = threadIdx.x % TPS), in R: wave shuffles of
// width TPS, and for a symbol of several waves (N >= 2048) the waves' pairs through the first reals of
// the symbol's row (`rr`; the caller's next sym_sync stands between these reads and the row's next
// writes).  Every lane of the symbol gets the result.
template <typename R, int TPS>
__device__ __forceinline__ void sym_sum_max(R& sum, R& mx, R* rr, int t) {
    constexpr int W = TPS < 64 ? TPS : 64;
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        const R o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if constexpr (TPS > 64) {
        sym_sync<TPS>();  // the IFFT's last pass has read the row
        if ((t & 63) == 0) {
            rr[2 * (t >> 6)] = sum;
            rr[2 * (t >> 6) + 1] = mx;
        }
        sym_sync<TPS>();
        sum = 0;
        mx = 0;
#pragma unroll
        for (int w = 0; w < TPS / 64; ++w) {
            sum += rr[2 * w];
            mx = rr[2 * w + 1] > mx ? rr[2 * w + 1] : mx;
        }
    }
}

// FB > 1: the throughput form (complex128 fixed square QAM of FB bits, cyclic-prefix OFDM, Philox
// streams); FB = 0: the generic form (any plan without an order above 256, caller bits or Philox)
template <typename R, int LOGN, int FB>
__global__ __launch_bounds__((papr_block<FB>()), (papr_waves<FB>())) void k_papr(PaprArgs a) {
    static_assert(FB == 0 || (sizeof(R) == 8 && FB > 1 && !(FB & 1) && uses_tt<R, LOGN, FB>()),
                  "throughput form: complex128 fixed square QAM, per-pass twiddles in LDS");
    constexpr int BLK = papr_block<FB>();
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr int N = G::N, E = G::E, TPS = G::TPS;
    constexpr bool TT = uses_tt<R, LOGN, FB>();
    constexpr int TTS = TT ? tt_size(LOGN) : 0;
    constexpr bool ROW_REAL = split_rows<R, FB>();
    const TxRxCommon& cm = a.c;
    const bool adaptive = FB ? false : (bool)cm.adaptive;
    const bool scm = FB ? false : (bool)cm.scm;  // SC-OFDM: no transform (run-time, uniform)
    const bool zp = FB ? false : (bool)cm.zpad;  // zero guard: counts in n, adds no power
    const int cp = cm.cp;
    constexpr int LUT_STATIC = FB > 1 ? (1 << FB) : 1;
    __shared__ C lut_s[LUT_STATIC];
    Carve cv(ofdm_smem);
    const PaprLds<R> lds = papr_carve<R, LOGN, FB>(cv, cm.lut_len, cm.words_per_sym);
    C *tw = lds.tw, *lut = FB > 0 ? lut_s : lds.lut, *tt = lds.tt;
    AxisInfo* axis = lds.axis;
    double* edges = lds.edges;
    uint32_t* hist = lds.hist;
    const int K = a.n_edges;

    // the tables' global reads issued first (Staged), then the LDS writes (as k_tx)
    Staged<BLK, TTS, C> st_tt;
    Staged<BLK, (FB > 0 ? LUT_STATIC : BLK), C, (FB > 0)> st_lut;  // (generic form: any LUT length)
    Staged<BLK, kMaxLuts, Dwords<AxisInfo>> st_ax;
    static_assert(kMaxLuts <= BLK, "one axis entry per thread");
    st_tt.load((const C*)cm.ptw + TTS, TTS);
    st_lut.load((const C*)cm.lut, cm.lut_len);
    st_ax.load((const Dwords<AxisInfo>*)cm.axis, cm.n_axis);
    if constexpr (!TT) load_twiddles<R>(tw, (const C*)cm.tw);
    // the 1/sqrt(N) of ifft(norm="ortho") folded into the LUT, and nothing else: no channel tap
    const R lut_scale = scm ? (R)1 : (R)cm.scale;
    st_tt.store(tt);
    st_lut.store(lut, [&](const C& v) { return cscale(v, lut_scale); });
    st_ax.store((Dwords<AxisInfo>*)axis);
    for (int i = threadIdx.x; i < K; i += BLK) edges[i] = a.edges[i];
    for (int i = threadIdx.x; i <= K; i += BLK) hist[i] = 0u;
    __syncthreads();

    const int ls = TPS >= 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x / TPS) : threadIdx.x / TPS;
    const int t = threadIdx.x % TPS;
    C* row = (C*)(lds.rowmem + (size_t)ls * G::PADN * (ROW_REAL ? sizeof(R) : sizeof(C)));
    uint32_t* W = lds.words + ls * cm.words_per_sym;
    const double nd = (double)(N + cp);  // samples per symbol, prefix or guard included
    const int64_t niter = (cm.n_sym + G::SPB - 1) / G::SPB;

    for (int64_t it = blockIdx.x; it < niter; it += gridDim.x) {
        const int64_t sl = it * G::SPB + ls;
        const int64_t sg = cm.sym0 + sl;
        const bool active = sl < cm.n_sym;
        TxBits<FB, TPS> tb;
        tb.load(cm, sg, t, W, active);
        if (FB == 0) sym_sync<TPS>();  // staged words visible
        // map (k_tx's statements; an inactive symbol of the throughput form maps its zero lane words
        // and is not binned)
        C x[E];
        if constexpr (FB > 0) {
            static_for<0, E>([&](auto I) { x[I] = lut[tb.template fixed<I>()]; });
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int k = t + i * TPS;
                C v = mk<R>(0, 0);
                if (active) {
                    if (adaptive) {
                        const ScInfo sc = cm.sc[k];
                        if (sc.lut >= 0) v = lut[axis[sc.lut].lut_off + tb.generic(i, sc.bits, sc.bitoff)];
                    } else {
                        v = lut[tb.generic(i, cm.b, k * cm.b)];
                    }
                }
                x[i] = v;
            }
        }
        if (!scm) fft_sym<R, LOGN, true, FB>(x, row, tw, tt, t);
        // the lane's share of the prefix (k_tx's prefix_sum rule): with cp <= TPS only its last element
        int ncp = N - cp;
        asm volatile("" : "+s"(ncp));
        auto prefix_sum = [&](auto&& pw) -> R {
            if (zp) return (R)0;  // the zero guard adds no power
            if (cp <= TPS) return t >= TPS - cp ? pw(E - 1) : (R)0;
            R acc = 0;
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (t + i * TPS >= ncp) acc += pw(i);
            return acc;
        };
        R pxs = 0, mxs = 0;  // per-symbol partials in the arithmetic precision
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const R p2 = norm2(x[i]);
            pxs += p2;
            mxs = FB > 0 ? peak_max(mxs, p2) : fmax(mxs, p2);
        }
        pxs += prefix_sum([&](int i) { return norm2(x[i]); });
        sym_sum_max<R, TPS>(pxs, mxs, (R*)row, t);
        if (active && t == 0) {
            // the bin: #{ i : peak n >= edges[i] sum } in double -- edges[i] sum is non-decreasing in
            // i (a rounded product by a non-negative factor is monotone), so the count is a bisection
            const double lhs = (double)mxs * nd, sd = (double)pxs;
            int lo = 0, hi = K;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (lhs >= edges[mid] * sd) lo = mid + 1;
                else hi = mid;
            }
            atomicAdd(&hist[lo], 1u);
            if (a.sym_out != nullptr && sl < a.sym_keep) {
                a.sym_out[2 * sl] = (double)mxs;
                a.sym_out[2 * sl + 1] = (double)pxs;
            }
        }
        sym_sync<TPS>();  // W / row reuse by the next symbol
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= K; i += BLK) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&a.hist[i], (unsigned long long)v);
    }
}

// Routing, the one definition: the throughput form takes the complex128 fixed-QAM bench shapes
// (bench_fixed_shape: cyclic-prefix OFDM or no prefix, FB = ref_fb > 1 -- 64-QAM at N = 1024, 256-QAM at
// N = 4096) on Philox streams; the generic form every other plan and any caller bits (the adaptive bench
// shape at N = 2048 among them).
template <typename R, int LOGN>
constexpr int papr_fb() {
    if constexpr (sizeof(R) == 8 && ref_fb<R, LOGN>() > 1) {
        if (uses_tt<R, LOGN, ref_fb<R, LOGN>()>()) return ref_fb<R, LOGN>();
    }
    return 0;
}
template <typename R, int LOGN>
static bool papr_fast_shape(const TxRxCommon& c) {
    if constexpr (papr_fb<R, LOGN>() == 0) return false;
    else return c.bits == nullptr && bench_fixed_shape<papr_fb<R, LOGN>()>(c);
}

template <typename R, int LOGN, int FB>
static hipError_t papr_launch(const PaprArgs& a, hipStream_t s) {
    constexpr int BLK = papr_block<FB>();
    using G = Geo<LOGN, BLK>;
    static_assert(G::SPB * G::TPS == BLK, "whole symbols per workgroup");
    CarveSize lds;
    papr_carve<R, LOGN, FB>(lds, a.c.lut_len, a.c.words_per_sym);
    if (lds.bytes + papr_static_lds<R, FB>() > kLdsPerCu) {
        // (a layout that does not fit: the generic form, which is the last resort)
        if constexpr (FB > 0) return papr_launch<R, LOGN, 0>(a, s);
        else return kLdsOverflow;
    }
    // every workgroup stages the edges and ends with an atomic per non-empty bin: two rounds of the
    // resident workgroups (as the profile's and the sweep's launchers)
    return rx_go<BLK, G::SPB>(k_papr<R, LOGN, FB>, lds.bytes, 2, a.c.n_sym, a, s);
}

template <typename R, int LOGN>
static hipError_t papr_one(const PaprArgs& a, hipStream_t s) {
    if constexpr (papr_fb<R, LOGN>() > 0) {
        if (papr_fast_shape<R, LOGN>(a.c)) return papr_launch<R, LOGN, papr_fb<R, LOGN>()>(a, s);
    }
    return papr_launch<R, LOGN, 0>(a, s);
}

template <typename R>
hipError_t launch_papr(int logn, const PaprArgs& a, hipStream_t s) {
    if (a.n_edges < 1 || a.n_edges > OFDM_MAX_PAPR_EDGES || a.hist == nullptr) return hipErrorInvalidValue;
    return with_logn(logn, [&](auto l) { return papr_one<R, decltype(l)::value>(a, s); });
}

#define OFDM_INSTANTIATE_PAPR(R) template hipError_t launch_papr<R>(int, const PaprArgs&, hipStream_t);

}  // namespace ofdm
