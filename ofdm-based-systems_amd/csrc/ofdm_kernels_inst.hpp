// ofdm_kernels_inst.hpp -- launcher definitions; included once per precision by
// ofdm_kernels_f32.hip / ofdm_kernels_f64.hip (explicit instantiation at the end of
// each), so the two precisions compile in parallel.
#pragma once

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "ofdm_kernels.hpp"

namespace ofdm {

// OFDM_AB_ONLY: experiment builds (Makefile VARIANT=..., tools/ab.sh) instantiate only the
// N = 1024..4096, 64/256-QAM and adaptive kernels of the bench configs -- a fraction of the
// full compile
#ifdef OFDM_AB_ONLY
#define OFDM_LOGN_CASES(X) X(10) X(11) X(12)
#define OFDM_FB_CASES(X) X(6) X(8)
#else
#define OFDM_LOGN_CASES(X) \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
// throughput kernels, both precisions: square QAM (4..256) and the reference's 4..32-PSK
#define OFDM_FB_CASES(X) X(2) X(3) X(4) X(5) X(6) X(8)
#endif

template <typename F>
static hipError_t set_smem(F fn, size_t bytes) {
    // Dynamic LDS above 64 KiB must be opted in per kernel; idempotent and cheap.
    (void)hipGetLastError();  // drop a stale error of an earlier, already-reported call
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

// a log2 N outside the build's cases: a plan never asks for one in a product build (N is checked at
// plan creation); an OFDM_AB_ONLY build lacks N < 1024 (kNotInBuild)
#ifdef OFDM_AB_ONLY
constexpr hipError_t kOutOfRange = kNotInBuild;
#else
constexpr hipError_t kOutOfRange = hipErrorInvalidValue;
#endif

// log2 N as a compile-time constant: f(std::integral_constant<int, L>) for the build's cases -- the
// one switch on logn of every launcher
template <typename F>
static hipError_t with_logn(int logn, F f) {
#define OFDM_LOGN_CASE(L) \
    case L:               \
        return f(std::integral_constant<int, L>{});
    switch (logn) {
        OFDM_LOGN_CASES(OFDM_LOGN_CASE)
        default:
            return kOutOfRange;
    }
#undef OFDM_LOGN_CASE
}
// c.eq as a compile-time constant: f(std::integral_constant<int, OFDM_EQ_*>)
template <typename F>
static hipError_t with_eq(int eq, F f) {
    if (eq == OFDM_EQ_NONE) return f(std::integral_constant<int, OFDM_EQ_NONE>{});
    if (eq == OFDM_EQ_ZF) return f(std::integral_constant<int, OFDM_EQ_ZF>{});
    return f(std::integral_constant<int, OFDM_EQ_MMSE>{});
}

constexpr int kFastMinLogN = 6;  // throughput specialisations for N >= 64

template <typename R, int LOGN, int MODE>
static hipError_t rows_one(const RowsArgs& a, hipStream_t s) {
    CarveSize lds;
    rows_carve<R, LOGN>(lds);
    const size_t sm = lds.bytes;
    auto fn = k_rows<R, LOGN, MODE>;
    static const hipError_t attr = set_smem(fn, sm);
    if (attr != hipSuccess) return attr;
    const int64_t groups = (a.n_rows + Geo<LOGN>::SPB - 1) / Geo<LOGN>::SPB;
    hipLaunchKernelGGL(fn, dim3(clamp_grid(groups)), dim3(kBlock), sm, s, a);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_rows(int logn, int mode, const RowsArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    return with_logn(logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if (mode == 0) return rows_one<R, L, 0>(a, s);
        if (mode == 1) return rows_one<R, L, 1>(a, s);
        return rows_one<R, L, 2>(a, s);
    });
}

// The elementwise kernels: `grid` workgroups of kBlock threads, no dynamic LDS (per_block: one
// workgroup per kBlock items of n); nothing to do for n <= 0
template <typename K, typename A>
static hipError_t launch_flat(K fn, int grid, const A& a, hipStream_t s) {
    (void)hipGetLastError();  // stale errors were reported by their own calls
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
template <typename K, typename A>
static hipError_t launch_flat_n(K fn, int64_t n, bool per_block, const A& a, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return launch_flat(fn, clamp_grid(per_block ? (n + kBlock - 1) / kBlock : n), a, s);
}

template <typename R>
hipError_t launch_equalize(const EqArgs& a, hipStream_t s) {
    return launch_flat_n(k_equalize<R>, a.n_rows, false, a, s);  // a workgroup per row
}
template <typename R>
hipError_t launch_map(const MapArgs& a, hipStream_t s) {
    return launch_flat_n(k_map<R>, a.n_out, true, a, s);
}
template <typename R>
hipError_t launch_demap(const DemapArgs& a, hipStream_t s) {
    return launch_flat_n(k_demap<R>, a.n_bytes, true, a, s);
}
template <typename R>
hipError_t launch_demap_count(const DemapCountArgs& a, hipStream_t s) {
    return launch_flat_n(k_demap_count<R>, a.n_sym * a.n_fft, true, a, s);
}
template <typename R>
hipError_t launch_conv(const ConvArgs& a, int grid, hipStream_t s) {
    return launch_flat(k_conv<R>, grid, a, s);
}
template <typename R>
hipError_t launch_power(const PowerArgs& a, int grid, hipStream_t s) {
    return launch_flat(k_power<R>, grid, a, s);
}
template <typename R>
hipError_t launch_awgn(const AwgnArgs& a, hipStream_t s) {
    return launch_flat_n(k_awgn<R>, a.len, true, a, s);
}

// Workgroups of a kernel resident on the device at once (occupancy x CUs), cached per kernel,
// device, workgroup size and dynamic LDS; 0 when the runtime cannot say.
template <typename F>
static int resident_blocks(F fn, int blk, size_t smem) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, int, size_t>, int> cached;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const auto key = std::make_tuple(reinterpret_cast<const void*>(fn), dev, blk, smem);
    std::lock_guard<std::mutex> lock(mu);
    const auto it = cached.find(key);
    if (it != cached.end()) return it->second;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), blk, smem) !=
            hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        return cached[key] = 0;
    }
    return cached[key] = per_cu * cus;
}

// Symbols per multipath symbol group (each group regenerates its predecessor's tail once): the
// chunk in [max / 2, max] whose rounds of resident workgroups times (chunk + 1) symbols per group
// is least.  A launch of 1e5 symbols (one point of an SNR sweep) at chunk 32 needed 1.5 rounds of
// workgroups -- two, the second half empty; chunk 25 fits it in two full rounds of 26-symbol
// groups instead of 33.
static inline int tx_chunk(int64_t n_sym, int max_chunk, int spb, int resident) {
    if (resident <= 0 || n_sym <= 0) return max_chunk;
    int best = max_chunk;
    int64_t best_cost = -1;
    for (int ch = max_chunk; ch >= (max_chunk + 1) / 2; --ch) {
        const int64_t blocks = ((n_sym + ch - 1) / ch + spb - 1) / spb;
        const int64_t cost = ((blocks + resident - 1) / resident) * (ch + 1);
        if (best_cost < 0 || cost < best_cost) best_cost = cost, best = ch;
    }
    return best;
}

// The tail of every fused transmitter launch (k_tx and its CLIP instantiations; tail: the kernel
// arguments behind TxArgs), after the launcher has sized the layout: `sm` bytes of dynamic LDS opted in,
// the multipath chunk fitted to whole rounds of the resident workgroups (tx_chunk), an uncapped grid of
// one workgroup per SPB symbol groups -- capping it at the resident workgroups, as rx_go does, cost the
// transmitter 4-8 % (profiles/r05h_ab_grid_resident.txt) -- returned in *grid, and the launch.
template <int BLK, int SPB, typename K, typename... T>
static hipError_t tx_go(K fn, size_t sm, TxArgs& a, int* grid, hipStream_t s, const T&... tail) {
    const hipError_t e = set_smem(fn, sm);
    if (e != hipSuccess) return e;
    const int resident = resident_blocks(fn, BLK, sm);
    if (a.chunk > 1) a.chunk = tx_chunk(a.c.n_sym, a.chunk, SPB, resident);
    const int64_t groups = (a.c.n_sym + a.chunk - 1) / a.chunk;
    *grid = clamp_grid((groups + SPB - 1) / SPB);
    hipLaunchKernelGGL(fn, dim3(*grid), dim3(BLK), sm, s, a, tail...);
    return hipGetLastError();
}

// WIDE: the generic kernel's instantiation for a plan with an order above 256 (a.wide set)
template <typename R, int LOGN, int FB, int LT, bool ZPW = false, bool REF = false, bool WIDE = false>
static hipError_t tx_launch(const TxArgs& a0, int* grid, hipStream_t s) {
    constexpr int BLK = tx_block<R, FB, LOGN, LT, ZPW>();
    if ((a0.wide != nullptr) != WIDE) return hipErrorInvalidValue;  // (tx_one sends a wide plan here, nothing else)
    TxArgs a = a0;
    a.slot = tx_row_slot<R, LOGN, FB, LT>(a.slot, a.c.cp);
    CarveSize lds;
    tx_carve<R, LOGN, FB, LT, BLK>(lds, a.c.lut_len, a.c.words_per_sym, tx_tails(a.L), a.slot,
                                   WIDE ? a.c.n_axis : 0);  // (a wide plan's level tables)
    const size_t sm = lds.bytes;
    if constexpr (FB > 0) {
        if (sm + tx_static_lds<R, FB, LT>() > kLdsPerCu) return tx_launch<R, LOGN, 0, -1>(a0, grid, s);
    } else {
        // the generic kernel is the last resort: a shape it cannot hold is refused, not launched
        if (sm + tx_static_lds<R, FB, LT>() > kLdsPerCu) return kLdsOverflow;
    }
    return tx_go<BLK, Geo<LOGN, BLK>::SPB>(k_tx<R, LOGN, FB, LT, ZPW, REF, WIDE>, sm, a, grid, s);
}

// throughput TX by channel length: flat / window FIR (<= 4 or <= 8 taps) / run-time taps (REF, see
// ref_shape: the generic kernel)
template <typename R, int LOGN, int FB, bool REF = false>
static hipError_t tx_fast(const TxArgs& a, int* grid, hipStream_t s) {
    constexpr int TPS = Geo<LOGN>::TPS;
    if (a.L == 1 && !a.c.zpad) return tx_launch<R, LOGN, FB, 0, false, REF>(a, grid, s);
    if constexpr (LOGN >= 8) {
        // the complex64 register window assumes a cyclic prefix; the complex128 one takes zero padding
        if (a.c.cp <= TPS && (!a.c.zpad || sizeof(R) == 8)) {
            // complex128 zero padding: the window FIR with the guard compiled in (ZPW)
            if constexpr (sizeof(R) == 8) {
                if (a.c.zpad) {
                    if (a.L <= 4) return tx_launch<R, LOGN, FB, 4, true>(a, grid, s);
                    if (a.L <= 8) return tx_launch<R, LOGN, FB, 8, true>(a, grid, s);
                }
            }
            if (a.L <= 4) return tx_launch<R, LOGN, FB, 4, false, REF>(a, grid, s);
            if (a.L <= 8) return tx_launch<R, LOGN, FB, 8, false, REF>(a, grid, s);
        }
    }
    return tx_launch<R, LOGN, REF ? 0 : FB, -1>(a, grid, s);
}

// The routing predicates of every fused launcher (TX, RX, the profile's and the sweep's), defined here once.
//
// What the adaptive throughput kernels (FB = 1) take: adaptive bit loading over the reference's
// square-QAM LUTs (upat: orders <= 256), OFDM with a cyclic prefix
static inline bool adaptive_fast(const TxRxCommon& c) { return c.adaptive && c.upat && !c.scm && !c.zpad && !c.nn; }
// What the fixed-order throughput kernels (FB = b) take: fixed square QAM or the reference's
// 4/8/16/32-PSK (psk_m > 0; odd bits: its 8/32-PSK only), OFDM or SC-OFDM, cyclic prefix or zero padding
static inline bool fixed_fast(const TxRxCommon& c) {
    return !c.adaptive && (!c.nn || c.psk_m > 0) && (c.b % 2 == 0 || c.psk_m > 0);
}
// Philox bits and noise, no received-symbol tap, and no exact zero whose tie the reference's first-index
// rule decides (RxArgs::zero_tie: an MMSE plan with a null bin -- the throughput slicers round the origin
// as their constants happen to, the generic kernel's apply the rule): what every throughput receiver needs
static inline bool philox_streams(const RxArgs& a) {
    return a.c.bits == nullptr && a.nr == nullptr && a.z_out == nullptr && !a.zero_tie;
}

// The bench configs' shapes: complex128, OFDM with a cyclic prefix (or none) -- fixed 64-QAM at N = 1024
// (configs b, c: FB = 6), adaptive square-QAM loading at N = 2048 (config d: FB = 1), fixed 256-QAM at
// N = 4096 (config e: FB = 8); 0 = no bench shape at this N and precision.  They are the shapes that have
//   - REF instantiations of k_tx / k_rx (ref_shape: the caller's bits),
//   - throughput forms of k_rx_prof, k_rx_frames, k_rx_dens and k_rx_soft (ofdm_record_inst.hpp: Philox streams),
//   - throughput forms of k_rx_sweep (ofdm_sweep_inst.hpp: the fixed-QAM ones, FB > 1, only).
template <typename R, int LOGN>
constexpr int ref_fb() { return sizeof(R) == 8 ? (LOGN == 10 ? 6 : LOGN == 11 ? 1 : LOGN == 12 ? 8 : 0) : 0; }
// fixed square QAM of exactly FB bits, OFDM, cyclic prefix or none (the part of fixed_fast without
// PSK, SC-OFDM and zero padding, at one order)
template <int FB>
static bool bench_fixed_shape(const TxRxCommon& c) {
    static_assert(FB > 1 && FB % 2 == 0, "a square-QAM order");
    return !c.adaptive && !c.nn && c.psk_m == 0 && c.b == FB && !c.scm && !c.zpad;
}
template <typename R, int LOGN>
static bool bench_shape(const TxRxCommon& c) {
    constexpr int FB = ref_fb<R, LOGN>();
    if constexpr (FB == 0) return false;
    else if constexpr (FB == 1) return adaptive_fast(c);
    else return bench_fixed_shape<FB>(c);
}

// Reference streams (the caller's bits; RX: and normals) on a bench shape, flat or <= 8-tap channels
// within the window FIR's reach, go through the throughput kernels' REF instantiations -- the timed
// kernels' bodies with the bit and noise source swapped (ref_lane, array normals) -- so the reference's
// own streams pin the benched FFT / FIR / slicer / count code (tests/test_gpu_ref_streams.py).
// Everything else with caller bits takes the generic kernel.
// Orders above 256 (1024- / 4096-QAM, wide PSK) always do, by the rules above as they stand: upat is
// false for a side above 16 (adaptive_fast), a bench shape has b = FB <= 8, and the FB switch has no
// case above 8 -- and the ABI refuses such a plan without caller bits before any launcher runs.
template <typename R, int LOGN>
static bool ref_shape(const TxRxCommon& c) { return c.bits != nullptr && bench_shape<R, LOGN>(c); }

// Throughput configuration (Philox bits, N >= 64): fixed_fast -> the kernel specialised on the bits
// per subcarrier; adaptive_fast -> the adaptive throughput kernel (FB = 1); anything else -> the
// generic kernel.
template <typename R, int LOGN>
static hipError_t tx_one(const TxArgs& a, int* grid, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        if (ref_shape<R, LOGN>(a.c)) return tx_fast<R, LOGN, ref_fb<R, LOGN>(), true>(a, grid, s);
    }
    if constexpr (LOGN >= kFastMinLogN) {
        if (a.c.bits == nullptr && adaptive_fast(a.c)) return tx_fast<R, LOGN, 1>(a, grid, s);
        if (a.c.bits == nullptr && fixed_fast(a.c)) {
#define OFDM_TX_FB(F) \
    case F:           \
        return tx_fast<R, LOGN, F>(a, grid, s);
            switch (a.c.b) {
                OFDM_FB_CASES(OFDM_TX_FB)
                default: break;
            }
#undef OFDM_TX_FB
        }
    }
    // the generic kernel; a plan with an order above 256 its WIDE instantiation
    if (a.wide != nullptr) return tx_launch<R, LOGN, 0, -1, false, false, true>(a, grid, s);
    return tx_launch<R, LOGN, 0, -1>(a, grid, s);
}

template <typename R>
hipError_t launch_tx(int logn, const TxArgs& a, int* grid, hipStream_t s) {
    return with_logn(logn, [&](auto l) { return tx_one<R, decltype(l)::value>(a, grid, s); });
}

// The tail of every fused receiver launch (k_rx, k_rx_prof, k_rx_sweep, k_link, k_papr), after the
// launcher has sized the layout: `sm` bytes of dynamic LDS opted in, a grid of ceil(n_sym / SPB)
// workgroups capped at `rounds` rounds of the workgroups resident at once, each then looping over its
// share of the symbols (rounds = 0, or a runtime that cannot say: uncapped up to kMaxGrid), and the launch.
// (tail: the kernel arguments behind `a`, as tx_go's -- k_rx_frames' RxFramesTail)
template <int BLK, int SPB, typename K, typename A, typename... T>
static hipError_t rx_go(K fn, size_t sm, int rounds, int64_t n_sym, const A& a, hipStream_t s, const T&... tail) {
    const hipError_t e = set_smem(fn, sm);
    if (e != hipSuccess) return e;
    int64_t want = (n_sym + SPB - 1) / SPB;
    const int res = rounds > 0 ? resident_blocks(fn, BLK, sm) : 0;
    if (res > 0) want = std::min<int64_t>(want, (int64_t)rounds * res);
    hipLaunchKernelGGL(fn, dim3(clamp_grid(want)), dim3(BLK), sm, s, a, tail...);
    return hipGetLastError();
}

// A form's kernel (RxForm, ofdm_fused.hpp) and the receiver's arguments inside the form's first kernel argument
template <RxForm F, typename R, int LOGN, int EQ, int FB, bool MV, bool REF, bool WIDE>
static auto rx_kernel() {
    static_assert(F == RxForm::Plain || !REF, "the REF instantiations have no record and no sweep");
    if constexpr (F == RxForm::Plain) return k_rx<R, LOGN, EQ, FB, MV, REF, WIDE>;
    else if constexpr (F == RxForm::Prof) return k_rx_prof<R, LOGN, EQ, FB, MV, false, WIDE>;
    else if constexpr (F == RxForm::Frames) return k_rx_frames<R, LOGN, EQ, FB, MV, WIDE>;
    else if constexpr (F == RxForm::Dens) return k_rx_dens<R, LOGN, EQ, FB, MV, WIDE>;
    else if constexpr (F == RxForm::Soft) return k_rx_soft<R, LOGN, EQ, FB, MV, WIDE>;
    else if constexpr (F == RxForm::Sweep) return k_rx_sweep<R, LOGN, EQ, FB, MV>;
    else return k_rx_sweep_frames<R, LOGN, EQ, FB, MV>;
}
static inline const RxArgs& rx_of(const RxArgs& a) { return a; }
static inline const RxArgs& rx_of(const RxSweepArgs& a) { return a.r; }
static inline int rx_points(const RxArgs&) { return 0; }
static inline int rx_points(const RxSweepArgs& a) { return a.n_snr; }

// The one "size, fall back, go" of every receiver form (rx_launch, rx_record_launch, rx_sweep_launch): the
// layout sized as the kernel carves it, by the form's own facts (RxFormOf: the workgroup shape; the sweep's
// points inside rx_carve; the density's histogram behind the layout; the profile's LUT pool in static LDS);
// a throughput layout that does not fit falls back to the generic kernel (EQ = -1, FB = 0, which builds
// the modem variants in), and the generic kernel is the last resort: a shape it cannot hold is refused, not
// launched (as tx_launch).  Then rx_go with the form's rounds.
// a: RxArgs, or the sweeps' RxSweepArgs; tail: the kernel arguments behind it (RxFramesTail, RxDensTail,
// RxSoftTail)
template <RxForm F, typename R, int LOGN, int EQ, int FB, bool MV, bool REF = false, bool WIDE = false, typename A,
          typename... T>
static hipError_t rx_form_launch(const A& a, hipStream_t s, T... tail) {
    using FORM = RxFormOf<F>;
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, FORM::ONE_WAVE>();
    using G = Geo<LOGN, BLK>;
    const TxRxCommon& c = rx_of(a).c;
    CarveSize lds;
    // (the profile's symbol slots reuse the FFT rows and the frame records need none: no dynamic LDS
    // beyond the receiver's own)
    rx_carve<R, LOGN, EQ, FB, MV, FORM::ONE_WAVE>(lds, c.words_per_sym, rx_tts<R, LOGN, FB>(c.scm), WIDE ? c.n_axis : 0,
                                                  rx_points(a));
    // the histogram behind the receiver's own layout, as the kernel carves it
    if constexpr (FORM::DENS) (dens_lds(lds, tail.bins), ...);
    // the soft record's level table and histogram likewise
    if constexpr (FORM::SOFT) (soft_lds(lds, tail.bins), ...);
    constexpr size_t lut = FORM::PROF ? prof_lut_static<FB>() * sizeof(cpx<R>) : 0;
    if (lds.bytes + rx_static_lds<R, FB>() + lut > kLdsPerCu) {
        if constexpr (FB > 0) return rx_form_launch<F, R, LOGN, -1, 0, true>(a, s, tail...);
        else return kLdsOverflow;
    }
    // one iteration of a workgroup bins at most SPB * N points (<= 16384): the 32-bit bins are flushed
    // every `flush` iterations, before any of them could reach 2^32 (k_rx_dens) -- by the shape launched
    if constexpr (FORM::DENS) ((tail.flush = (uint32_t)(0xFFFFFFFFull / ((unsigned long long)G::SPB * G::N))), ...);
    // (the soft record: one iteration puts at most one bit of each of its SPB * N elements into one bin)
    if constexpr (FORM::SOFT) ((tail.flush = (uint32_t)(0xFFFFFFFFull / ((unsigned long long)G::SPB * G::N))), ...);
    // Two rounds of the resident workgroups where every workgroup ends with atomics of its own: up to five
    // per subcarrier (profile), up to one per bin (density), a pair per point behind a table per point
    // (the sweeps).  The frame record adds none per workgroup: k_rx's own grid.
    constexpr int rounds = FORM::PROF || FORM::DENS || FORM::SWEEP || FORM::SOFT ? 2 : rx_grid_rounds<R, FB, LOGN>();
    return rx_go<BLK, G::SPB>(rx_kernel<F, R, LOGN, EQ, FB, MV, REF, WIDE>(), lds.bytes, rounds, c.n_sym, a, s, tail...);
}

template <typename R, int LOGN, int EQ, int FB, bool MV, bool REF = false, bool WIDE = false>
static hipError_t rx_launch(const RxArgs& a, hipStream_t s) {
    if ((a.wide != nullptr) != WIDE) return hipErrorInvalidValue;  // (as tx_launch)
    return rx_form_launch<RxForm::Plain, R, LOGN, EQ, FB, MV, REF, WIDE>(a, s);
}

// MV: the run-time modem variants (SC-OFDM, zero padding) compiled in.  complex128 builds them as
// separate kernels: compiled into the cyclic-prefix OFDM kernels of the bench, their second
// transform and guard overlap-add spilled the config (b) receiver (~70 dwords at 128 VGPRs)
template <typename R, int LOGN, int FB, bool MV = true, bool REF = false>
static hipError_t rx_eq(const RxArgs& a, hipStream_t s) {
    return with_eq(a.c.eq, [&](auto eq) { return rx_launch<R, LOGN, decltype(eq)::value, FB, MV, REF>(a, s); });
}

// Throughput configuration (Philox bits and noise, no received-symbol tap; N >= 64): fixed_fast ->
// the kernel specialised on bits and equaliser; adaptive_fast -> the adaptive one; anything else ->
// the generic kernel.
template <typename R, int LOGN>
static hipError_t rx_one(const RxArgs& a, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        // reference streams on a bench shape (see ref_shape): the REF receiver needs the caller's
        // normals and no received-symbol tap
        // (MV: as the timed kernels -- compiled out of the fixed-QAM ones, and in the adaptive
        // kernel's instantiation, where FB = 1 forces SC-OFDM and zero padding off)
        // (and, as philox_streams, no tie at the origin to decide)
        if (ref_shape<R, LOGN>(a.c) && a.nr != nullptr && a.z_out == nullptr && !a.zero_tie)
            return rx_eq<R, LOGN, ref_fb<R, LOGN>(), ref_fb<R, LOGN>() == 1, true>(a, s);
    }
    if constexpr (LOGN >= kFastMinLogN) {
        const bool streams = philox_streams(a);
        if (streams && adaptive_fast(a.c)) return rx_eq<R, LOGN, 1>(a, s);
        if (streams && fixed_fast(a.c)) {
#define OFDM_RX_FB(F)                                                                      \
    case F:                                                                                \
        if constexpr (sizeof(R) == 8) { /* the modem variants in kernels of their own: rx_eq */ \
            if (!a.c.scm && !a.c.zpad) return rx_eq<R, LOGN, F, false>(a, s);        \
        }                                                                                  \
        return rx_eq<R, LOGN, F, true>(a, s);
            switch (a.c.b) {
                OFDM_FB_CASES(OFDM_RX_FB)
                default: break;
            }
#undef OFDM_RX_FB
        }
    }
    if (a.wide != nullptr) return rx_launch<R, LOGN, -1, 0, true, false, true>(a, s);  // (as tx_one)
    return rx_launch<R, LOGN, -1, 0, true>(a, s);
}

template <typename R>
hipError_t launch_rx(int logn, const RxArgs& a, hipStream_t s) {
    return with_logn(logn, [&](auto l) { return rx_one<R, decltype(l)::value>(a, s); });
}

// The launchers are instantiated in three groups so the complex64 kernels -- the bulk of
// the compile -- build as separate translation units in parallel (ofdm_kernels_f32*.hip).
#define OFDM_INSTANTIATE_OPS(R)                                                     \
    template hipError_t launch_rows<R>(int, int, const RowsArgs&, hipStream_t);     \
    template hipError_t launch_equalize<R>(const EqArgs&, hipStream_t);             \
    template hipError_t launch_map<R>(const MapArgs&, hipStream_t);                 \
    template hipError_t launch_demap<R>(const DemapArgs&, hipStream_t);             \
    template hipError_t launch_demap_count<R>(const DemapCountArgs&, hipStream_t);  \
    template hipError_t launch_conv<R>(const ConvArgs&, int, hipStream_t);          \
    template hipError_t launch_power<R>(const PowerArgs&, int, hipStream_t);        \
    template hipError_t launch_awgn<R>(const AwgnArgs&, hipStream_t);
#define OFDM_INSTANTIATE_TX(R) template hipError_t launch_tx<R>(int, const TxArgs&, int*, hipStream_t);
#define OFDM_INSTANTIATE_RX(R) template hipError_t launch_rx<R>(int, const RxArgs&, hipStream_t);
#define OFDM_INSTANTIATE(R) OFDM_INSTANTIATE_OPS(R) OFDM_INSTANTIATE_TX(R) OFDM_INSTANTIATE_RX(R)

}  // namespace ofdm
