// ofdm_fused.hpp -- the two fused hot-path kernels (included by ofdm_kernels.hpp).
//
// Data distribution: a symbol is owned by TPS = N/E threads; thread t holds
// elements k = t + i*TPS (i < E) in registers from the constellation map through
// the IFFT to the channel output (TX), and from the HBM load through the FFT to
// the error count (RX).  LDS carries only the Stockham transposes between FFT
// passes, (reference mode) the symbol's tx bit words, and (TX, multipath) the
// extended serial stream for the FIR.  With TPS <= 64 a symbol lives in one
// wavefront and every synchronisation is wave-local (sym_sync), so the 4 waves of a
// workgroup run decoupled.
//
// Specialisations: FB = 2/4/6/8 selects the throughput kernel (fixed square QAM -- or the
// reference's 4/16-PSK -- with b = FB bits, Philox-keyed bits and noise, complex64; OFDM or
// SC-OFDM, cyclic prefix or zero padding as wave-uniform run-time flags); FB = 3/5 the same
// kernel for the reference's 8/32-PSK (sector decisions only); FB = 1 is the throughput kernel for adaptive
// bit loading (per-subcarrier square-QAM orders, CAPACITY_BASED, OFDM with a cyclic prefix);
// FB = 0 is the generic kernel (reference-mode bytes and normals, PSK, complex128, adaptive
// SC-OFDM / zero padding); its WIDE instantiation serves plans with a constellation above 256
// points (1024- / 4096-QAM, wide PSK): per-axis level tables instead of a LUT staged in LDS.
#pragma once

#include <algorithm>
#include <type_traits>

// Minimum waves per SIMD requested per fused kernel (register budget 512/waves), tuned on
// MI355X (tools/ab.sh): TX 3 waves/SIMD, RX unconstrained.  Build-time knobs (Makefile
// TX_WAVES / RX_WAVES) for occupancy studies.
#ifndef OFDM_TX_WAVES
#define OFDM_TX_WAVES 3
#endif
// throughput TX with the register-window FIR (LT = 4 / 8): 2 waves/SIMD (256 registers) --
// at 3 the window, the taps and the FFT state spill (54 VGPRs at LT = 8); measured on MI355X:
// config (c) TX 3.71 -> 2.94 ms, (e) 14.1 -> 12.5 ms per 1e6 symbols, while the generic kernel
// is faster at 3 (SC-OFDM TX 3.57 vs 4.33 ms)
#ifndef OFDM_TX_WFIR_WAVES
#define OFDM_TX_WFIR_WAVES 2
#endif
#ifndef OFDM_RX_WAVES
#define OFDM_RX_WAVES 1
#endif
// Workgroup of the throughput (FB > 0) kernels at N <= 1024 (TX; RX without equaliser):
// 8 waves share one copy of the twiddle tables and two workgroups fit the 160 KB LDS, i.e.
// 4 waves per SIMD (register budget 128).  Other variants: 256 threads, OFDM_*_WAVES.
#ifndef OFDM_TX_FAST_BLOCK
#define OFDM_TX_FAST_BLOCK 512
#endif
#ifndef OFDM_RX_FAST_BLOCK
#define OFDM_RX_FAST_BLOCK 512
#endif

// Streaming (nontemporal) loads of the channel samples in RX: y is read exactly once, and
// the nontemporal hint lifts the achievable read rate of this access pattern on MI355X from
// 6.2 to 7.1 TB/s (tools/hbm_probe.hip).  TX stores: the same hint, off for complex64 (no gain
// measured on the write side), on for the complex128 flat TX (config b TX 3.10 -> 3.00 ms,
// profiles/r03r_ab.txt; not on the window-FIR TX's lane-contiguous stores).
#ifndef OFDM_RX_NT
#define OFDM_RX_NT 1
#endif
#ifndef OFDM_TX_NT
#define OFDM_TX_NT 0
#endif
#ifndef OFDM_TX_NT_F64
#define OFDM_TX_NT_F64 1
#endif

namespace ofdm {

template <bool NT, typename C>
__device__ __forceinline__ C ld_stream(const C* p) {
    if constexpr (NT && sizeof(C) == 8) {
        C v;
        v.v = __builtin_nontemporal_load((const f32x2*)p);
        return v;
    } else if constexpr (NT && sizeof(C) == 16) {
        const f64x2 u = __builtin_nontemporal_load((const f64x2*)p);
        C v;
        v.re = u.x;
        v.im = u.y;
        return v;
    } else {
        return *p;
    }
}
template <bool NT, typename C>
__device__ __forceinline__ void st_stream(C* p, C v) {
    if constexpr (NT && sizeof(C) == 8)
        __builtin_nontemporal_store(v.v, (f32x2*)p);
    else
        *p = v;
}
template <bool NT>
__device__ __forceinline__ void st_stream(__attribute__((address_space(1))) cpx<float>* p, cpx<float> v) {
    typedef __attribute__((address_space(1))) f32x2 gf2;
    if constexpr (NT)
        __builtin_nontemporal_store(v.v, (gf2*)p);
    else
        *(gf2*)p = v.v;
}
template <bool NT>
__device__ __forceinline__ void st_stream(__attribute__((address_space(1))) cpx<double>* p, cpx<double> v) {
    typedef __attribute__((address_space(1))) f64x2 gd2;
    const f64x2 u = f64x2{v.re, v.im};
    if constexpr (NT)
        __builtin_nontemporal_store(u, (gd2*)p);
    else
        *(gd2*)p = u;
}

// Global-memory (address space 1) pointers: a pointer rebuilt from an integer would
// otherwise be generic and compile to flat_* instructions.
template <typename T>
using gptr = __attribute__((address_space(1))) T*;

// A wave-uniform pointer held in SGPRs (readfirstlane of both halves).
template <typename T>
__device__ __forceinline__ gptr<T> uniform_ptr(T* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (gptr<T>)(((uint64_t)hi << 32) | lo);
}
// base + element offset as (64-bit base) + zext(32-bit byte offset): the addressing the
// global_load/store SGPR-base form matches
template <typename T>
__device__ __forceinline__ gptr<T> lane_ptr(gptr<T> base, uint32_t elem) {
    return (gptr<T>)((__attribute__((address_space(1))) char*)base + (uint64_t)(elem * (uint32_t)sizeof(T)));
}

// Raw buffer resource over `bytes` bytes at p (gfx9 word 3) and a 16-byte load at a lane byte
// offset (VGPR) plus a wave-uniform one (SGPR): one address register for any number of loads.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// (NT: the nontemporal hint, cache-policy bit 1 on gfx950)
template <typename T, bool NT = false>
__device__ __forceinline__ T buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    static_assert(sizeof(T) == 16, "16-byte element");
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, NT ? 2 : 0));
}
// (No buffer-store counterpart, deliberately: buffer_store_dwordx4 with a register SGPR offset
// corrupted the low data dword on gfx950 -- the compiler inserts no wait state between such a store
// and the next VALU write of its data VGPRs, DESIGN.md section 4.  Stores use the global_store forms;
// tests/test_isa_guard.py rejects any buffer store in the fused kernels' code.)

// complex128 multipath TX of square QAM (the plan sends only separable LUTs to the throughput
// kernels): map through the two axis tables instead of the complex LUT (TX c 5.13 -> 5.12, e 5.26
// -> 5.17 ms per step, profiles/r03aa_ab.txt)
template <typename R, int FB, int LT>
constexpr bool tx_sep_lut() { return sizeof(R) == 8 && FB >= 2 && !(FB & 1) && LT != 0; }

// complex128 RX with a symbol per wave: the channel samples through buffer loads (one address
// VGPR, the element offsets in SGPRs) instead of four 64-bit VGPR addresses (RX b 3.09 -> 3.06,
// c 3.75 -> 3.70 ms per step at the same occupancy, profiles/r03ab_ab.txt)

// MP: multipath channel (L > 1; the generic kernel always takes L from the plan)
#ifndef OFDM_TX_MP_BLOCK
#define OFDM_TX_MP_BLOCK 256
#endif
// complex128 throughput kernels (R = double, FB > 0).  The FFT exchanges through split real /
// imaginary rows (fft_reg_split: 8.5 KB per N = 1024 symbol), so the occupancy is set by the
// registers: 16 complex128 elements per lane plus a radix-16 butterfly -- RX ~160 VGPRs (3 waves
// per SIMD: one 768-thread workgroup of 12 symbols per CU), flat TX 128 (4 waves: 1024 threads).
// A 4-wave RX (1024 threads, 128 VGPRs, 7 spilled) measured config b 1.646 -> 1.648e8 symbols/s,
// within the run-to-run spread (profiles/r03k_ab_rx1024.txt); with the channel samples
// buffer-loaded (6 dwords spilled at 128) it gains: RX 3.09 -> 2.98 ms, 1.669 ->
// 1.693e8 symbols/s (profiles/r03ab_ab.txt) -- the no-equaliser RX takes 1024 threads at 4 waves.
// The window-FIR TX passes the extended stream through its row of reals twice (real, then
// imaginary parts), in 256-thread workgroups at 2 waves per SIMD: two or more workgroups per
// CU, so a symbol group's barriers (N >= 2048: TPS > 64) hold back fewer waves.  Against
// complex rows at 512 threads (256 where they did not fit, 1 wave per SIMD): TX per step
// c 5.45 -> 5.37, d 7.01 -> 5.41, e 6.37 -> 5.39 ms; rows of reals at 512 threads measured
// 5.59 / 6.67 / 6.65 (profiles/r03o_ab.txt).
#ifndef OFDM_F64_TX_BLOCK
#define OFDM_F64_TX_BLOCK 1024
#endif
#ifndef OFDM_F64_TX_WAVES
#define OFDM_F64_TX_WAVES 4
#endif
#ifndef OFDM_F64_RX_BLOCK
#define OFDM_F64_RX_BLOCK 1024
#endif
#ifndef OFDM_F64_RX_WAVES
#define OFDM_F64_RX_WAVES 4
#endif
#ifndef OFDM_F64_FIR_BLOCK
#define OFDM_F64_FIR_BLOCK 256
#endif
#ifndef OFDM_F64_FIR_WAVES
#define OFDM_F64_FIR_WAVES 2
#endif
// N = 4096 (config e, 4 waves per symbol): 3 waves per SIMD (168 VGPRs, 18 dwords spilled) --
// TX e 4.65 -> 4.46 ms, 2.833 -> 2.877e7 symbols/s (profiles/r04q_ab_e_fir_3waves.txt); at N = 1024 /
// 2048 the same step spills 39 / 51 dwords (config c measured 15 % slower, profiles/r04b_ab_fir.txt)
#ifndef OFDM_F64_FIR_WAVES_4K
#define OFDM_F64_FIR_WAVES_4K 3
#endif
// complex64 throughput kernels at N >= 2048 (configs d, e): workgroup and waves per SIMD of RX
// and of the window-FIR TX (two or four waves per symbol).  With the compact twiddle tables the
// LDS no longer caps a CU at two workgroups, so 3 waves per SIMD fit: config e RX 3.37 -> 2.84 ms
// per 2.5e5 symbols; N = 2048 (config d) prefers 768-thread workgroups (RX 3.08 -> 2.99 ms per
// 5e5 symbols), N = 4096 256 (profiles/r03h_ab.txt)
#ifndef OFDM_RX_BIG_BLOCK
#define OFDM_RX_BIG_BLOCK(LOGN) ((LOGN) == 11 ? 768 : 256)
#endif
#ifndef OFDM_RX_BIG_WAVES
#define OFDM_RX_BIG_WAVES 3
#endif
#ifndef OFDM_TX_BIG_WFIR_WAVES
#define OFDM_TX_BIG_WFIR_WAVES 3
#endif
// LDS per CU on gfx950.  The complex128 FIR TX sizes its workgroup against it (tx_block), and a
// throughput-kernel instantiation whose LDS would exceed it (a shape the plan allows but the
// specialised layout cannot hold) runs the generic kernel instead of failing at launch
// (tests/test_gpu_edges.py::test_lds_limit_shapes_run)
constexpr size_t kLdsPerCu = 160 * 1024;
// padded FIR row index of the throughput multipath TX: one slot per 16 elements
__host__ __device__ constexpr int fir_pad(int i) { return i + (i >> 4); }
// complex128 window-FIR TX, LDS slots (16 bytes) of the half-symbol row.  Stream phase: stream
// index kk at wfir_in(kk) -- one pad slot per 8, placed so that the FFT elements (kk = LT - 1 +
// t + TPS i mod 8: every 8 lanes one aligned run) are written without a pad inside an 8-lane
// group, and the lanes' windows (kk = 8 t + W) read at lane stride 9.  Output phase: output kk at
// wfir_out(kk), an XOR swizzle of the 8-slot runs -- the lanes' runs of 8 outputs are written to
// distinct banks and the stores' reads (kk = t + TPS i) hit 16 distinct 4-bank sets per
// ds_read_b128 lane group.  Against wfir_slot (kk + kk / 8) for both phases: no bank conflicts
// (SQ_LDS_BANK_CONFLICT 197 cycles per config-c symbol, tools/lds_banks.py --fir models 192).
__host__ __device__ constexpr int wfir_ioff(int lt) { return (9 - lt) & 7; }
__host__ __device__ constexpr int wfir_in(int kk, int lt) { return kk + ((kk + wfir_ioff(lt)) >> 3); }
__host__ __device__ constexpr int wfir_out(int kk) { return (kk & ~7) | ((kk ^ (kk >> 3)) & 7); }
// complex128 RX of fixed QAM at N = 4096 (config e): one symbol per 256-thread workgroup at 3 waves
// per SIMD, the equaliser coefficients read from the plan's table after the FFT (rx_eq_late)
// instead of a 64 KB LDS copy per workgroup -- with the copy, two symbols per 512-thread workgroup
// at 2 waves per SIMD, one barrier coupling both symbols' FFT exchanges.  Config e RX 5.02 ->
// 4.21 ms per 2.5e5 symbols (2 waves per SIMD: 4.63); the step gains less (9.99 -> 9.64 ms): the
// TX that follows runs 0.4 ms slower at the power cap (profiles/r03y_ab.txt)
#ifndef OFDM_F64_RX_SOLO_WAVES
#define OFDM_F64_RX_SOLO_WAVES 3
#endif
// the complex128 adaptive receiver at N = 2048 (config d): one 128-thread symbol per workgroup
#ifndef OFDM_F64_RX_ADAPT_WAVES
#define OFDM_F64_RX_ADAPT_WAVES 2
#endif
// the OFDM_F64_RX_BLOCK / _WAVES shape: no-equaliser RX of 64/256-QAM at N = 1024 (at 128 VGPRs the
// QPSK / 16-QAM and smaller-N kernels spill 22-33 dwords, so they stay at 768 threads, 3 waves;
// with an equaliser the 16 KB coefficient table beside 16 symbols' rows exceeds the LDS)
template <int FB, int LOGN, int EQ, bool MV = false>
constexpr bool f64_rx_wide() { return EQ == OFDM_EQ_NONE && FB >= 6 && LOGN == 10 && !MV; }
// (the same for the adaptive RX at N = 2048 (config d) -- 128-thread workgroups
// of one symbol at 2 waves per SIMD, instead of four symbols per 512-thread workgroup: RX 5.12 ->
// 4.67 ms, step 10.11 -> 9.93 ms per 5e5 symbols, profiles/r03ad_ab.txt)
template <typename R, int FB, int LOGN>
constexpr bool f64_rx_solo() {
    return sizeof(R) == 8 && ((FB > 1 && LOGN == 12) || (FB == 1 && LOGN == 11));
}
// The six receiver forms, named once, and each form's compile-time facts: what its kernel states in
// __launch_bounds__ and in its `constexpr bool PROF, SWEEP, FRAMES, DENS` line, what the body
// (ofdm_rx_body.hpp) sizes its workgroup and carves its LDS by, and what the launcher (rx_form_launch,
// ofdm_kernels_inst.hpp) sizes, routes and launches by -- one description, so the three cannot disagree.
enum class RxForm { Plain, Prof, Frames, Dens, Sweep, SweepFrames, Soft };
template <RxForm F>
struct RxFormOf {
    static constexpr bool PROF = F == RxForm::Prof;                               // k_rx_prof
    static constexpr bool SWEEP = F == RxForm::Sweep || F == RxForm::SweepFrames;    // k_rx_sweep, k_rx_sweep_frames
    static constexpr bool FRAMES = F == RxForm::Frames || F == RxForm::SweepFrames;  // k_rx_frames, k_rx_sweep_frames
    static constexpr bool DENS = F == RxForm::Dens;                               // k_rx_dens
    // one wave per SIMD: the workgroup shape of rx_block / rx_waves / rx_carve (the reasons: rx_block)
    static constexpr bool SOFT = F == RxForm::Soft;                               // k_rx_soft
    static constexpr bool ONE_WAVE = PROF || SWEEP || DENS || SOFT;
};
// MV: the complex128 SC-OFDM / zero-padding kernels (k_rx MV), ~10-50 VGPRs above their cyclic-prefix
// OFDM twins: never the 4-wave shape, and the one-symbol N = 4096 shape at 2 waves per SIMD
// ONE_WAVE (RxFormOf, below): a throughput receiver with the per-subcarrier profile (k_rx_prof) keeps five
// accumulators per element (~110 VGPRs) beside the kernel's own 130-200, so it runs at one wave per SIMD:
// 256 threads (the one-symbol shapes as they are) instead of the 512 - 1024-thread shapes tuned to
// 128 - 168 registers.  The sweep's throughput form (k_rx_sweep, k_rx_sweep_frames) takes the shape for the
// y (64 VGPRs), the radii and the phase words it holds in registers across the points, and the density's
// (k_rx_dens) because the throughput receivers fill the LDS at their own shapes (about 156 of 160 KB at
// config b's) and this one leaves the histogram its 64 KB.
template <typename R, int FB, int LOGN, int EQ, bool MV, bool ONE_WAVE>
constexpr int rx_block() {
    if (ONE_WAVE && FB > 0) return f64_rx_solo<R, FB, LOGN>() ? (1 << LOGN) / 16 : 256;
    // (the adaptive kernel's per-order tables take ~200 VGPRs in complex128: 2 waves per SIMD)
    if (f64_rx_solo<R, FB, LOGN>()) return (1 << LOGN) / 16;  // one symbol
    if (sizeof(R) == 8 && FB > 0)
        return (LOGN > 10 || FB == 1) ? 512 : (f64_rx_wide<FB, LOGN, EQ, MV>() ? OFDM_F64_RX_BLOCK : 768);
    if (FB > 0 && LOGN > 10) return OFDM_RX_BIG_BLOCK(LOGN);
    return FB > 1 && LOGN <= 10 && EQ == OFDM_EQ_NONE ? OFDM_RX_FAST_BLOCK : kBlock;
}
template <typename R, int FB, int LOGN, int EQ, bool MV, bool ONE_WAVE>
constexpr int rx_waves() {
    if (ONE_WAVE && FB > 0) return 1;
    if (f64_rx_solo<R, FB, LOGN>()) return FB == 1 ? OFDM_F64_RX_ADAPT_WAVES : MV ? 2 : OFDM_F64_RX_SOLO_WAVES;
    if (sizeof(R) == 8 && FB > 0)
        return (LOGN > 10 || FB == 1) ? 2 : (f64_rx_wide<FB, LOGN, EQ, MV>() ? OFDM_F64_RX_WAVES : 3);
    if (FB > 0 && LOGN > 10) return OFDM_RX_BIG_WAVES;
    return rx_block<R, FB, LOGN, EQ, MV, ONE_WAVE>() >= 512 ? 4 : OFDM_RX_WAVES;
}
// throughput RX: equaliser coefficients staged in LDS up to N = 2^OFDM_EQ_LDS_MAX_LOGN (beyond,
// the table would cost a resident workgroup per CU)
#ifndef OFDM_EQ_LDS_MAX_LOGN
#define OFDM_EQ_LDS_MAX_LOGN 11
#endif
// complex128 at N = 4096: the table (64 KB) fits beside two symbols' split rows and the compact
// twiddles, and preloading 16 complex128 coefficients would spill
template <typename R, int FB, int LOGN, int EQ>
constexpr bool eq_in_lds() {
    return FB > 0 && EQ > OFDM_EQ_NONE && LOGN <= (sizeof(R) == 8 ? 12 : OFDM_EQ_LDS_MAX_LOGN) &&
           !f64_rx_solo<R, FB, LOGN>();
}
// complex128 throughput receivers at N = 1024 (configs b, c): one workgroup holds a CU, and each
// start and drain of one idles it -- the grid is OFDM_RX_GRID_ROUNDS rounds of the resident
// workgroups instead of up to kMaxGrid.  Config c RX 3.556 -> 3.50 ms per 1e6 symbols and
// 0.43 -> 0.37 ms per 1e5 (a sweep point); one round (static striding) lost 2 % at 1e6, and the
// other receivers (several workgroups per CU) lost 1-5 % with two (profiles/r05h_ab_grid_resident.txt).
// (A queue the waves took their symbols from was 3.4x slower: one atomic counter serialised
// ~12 ns per symbol, profiles/r05j_ab_rx_symbol_queue.txt.)
#ifndef OFDM_RX_GRID_ROUNDS
#define OFDM_RX_GRID_ROUNDS 2
#endif
template <typename R, int FB, int LOGN>
constexpr int rx_grid_rounds() {
    return sizeof(R) == 8 && FB > 0 && LOGN == 10 ? OFDM_RX_GRID_ROUNDS : 0;
}
// the lane's coefficients loaded after the FFT (in flight across the MMSE power reduction)
template <typename R, int FB, int LOGN, int EQ>
constexpr bool rx_eq_late() { return f64_rx_solo<R, FB, LOGN>() && EQ > OFDM_EQ_NONE; }
// MMSE in complex128: the reciprocals of |H|^2 + nv of four elements from one v_rcp_f64 (+ two
// Newton steps) and nine products (Montgomery's batch inversion; ~3 roundings more than one
// reciprocal each, well inside the decision bracket's 8 u of equaliser arithmetic).  RX c 3.80 ->
// 3.75, e 4.21 -> 4.16 ms per step (profiles/r03y_ab.txt)
// complex128 throughput kernels exchange FFT data through rows of reals (fft_reg_split)
template <typename R, int FB>
constexpr bool split_rows() { return sizeof(R) == 8 && FB > 0; }


// Reference mode: stage OFDM symbol s's tx bits from the packed bytes of the run
// (symbol s starts at bit s*bps, zeros past the end) as 32-bit words in W
// (stream bit 32w+j = bit 31-j of word w).  Returns the symbol's bit offset in word 0.
template <int TPS>
__device__ __forceinline__ int stage_words(const TxRxCommon& a, int64_t s, uint32_t* W, int t) {
    const int64_t bit0 = s * a.bps;
    const int64_t B0 = bit0 >> 3;
    for (int w = t; w < a.words_per_sym; w += TPS) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t B = B0 + 4 * w + i;
            v = (v << 8) | (uint32_t)((B < a.n_bytes && s >= 0) ? a.bits[B] : 0);
        }
        W[w] = v;
    }
    return (int)(bit0 & 7);
}

template <typename R>
__device__ __forceinline__ R recip(R d) {
    if constexpr (sizeof(R) == 4) {
        return __builtin_amdgcn_rcpf(d);  // v_rcp_f32 (1 ulp): throughput mode
    } else {
        // v_rcp_f64 and two Newton steps (~1 ulp) instead of the IEEE division sequence
        R r = __builtin_amdgcn_rcp(d);
        r = __builtin_fma(__builtin_fma(-d, r, (R)1), r, r);
        return __builtin_fma(__builtin_fma(-d, r, (R)1), r, r);
    }
}

// MMSE filter coefficient conj(H)/(|H|^2 + nv) (equalization/models.py:58-61).  In f64 the
// two divisions of the reference are kept; in f32 one reciprocal.
template <typename R>
__device__ __forceinline__ cpx<R> mmse_coef(cpx<R> hc, R h2, R nv) {
    const R d = h2 + nv;
    if constexpr (sizeof(R) == 4) {
        const R inv = recip<R>(d);
        return mk<R>(hc.re * inv, hc.im * inv);
    } else {
        return mk<R>(hc.re / d, hc.im / d);
    }
}

// The lane block of a reference-stream symbol for the throughput kernels' REF instantiations: byte
// i = the FB bits of element i (subcarrier k = t + i TPS), read MSB first from the caller's byte
// stream at bit s bps + k FB (the reference's bit order, bits_generation/models.py:26-44 and
// serial_parallel/models.py:12-33) -- the layout lane_bits reads, so the kernel body is the
// throughput kernel's.  Global byte reads (uncoalesced: REF runs are parity runs, not timed).
template <int FB, int TPS>
__device__ __forceinline__ u4 ref_lane(const TxRxCommon& a, int64_t s, int t) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const int64_t bit0 = s * a.bps;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t o = bit0 + (int64_t)(t + i * TPS) * FB;
        const int64_t B = o >> 3;
        const uint32_t hi = B < a.n_bytes ? (uint32_t)a.bits[B] : 0u;
        const uint32_t lo = B + 1 < a.n_bytes ? (uint32_t)a.bits[B + 1] : 0u;
        const uint32_t v = (((hi << 8) | lo) >> (16 - (int)(o & 7) - FB)) & ((1u << FB) - 1u);
        w[i >> 2] |= v << (8 * (i & 3));
    }
    return u4{w[0], w[1], w[2], w[3]};
}

// The same for adaptive loading (FB = 1): byte i = the b_k bits of subcarrier k = t + i TPS, read MSB
// first at bit s bps + bitoff_k (constellation/adaptive.py:178-199: each OFDM symbol's bits laid out
// subcarrier-major with variable b_k), zero for an unused subcarrier -- the lane byte the adaptive
// kernels mask with (1 << b_k) - 1.  b_k <= 8 (the plan's upat: orders <= 256), so three bytes cover
// any alignment.
template <int TPS>
__device__ __forceinline__ u4 ref_lane_adaptive(const TxRxCommon& a, int64_t s, int t) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    const int64_t bit0 = s * a.bps;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const ScInfo sc = a.sc[t + i * TPS];
        if (sc.lut < 0 || sc.bits <= 0) continue;
        const int64_t o = bit0 + sc.bitoff;
        const int64_t B = o >> 3;
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) v = (v << 8) | (B + j < a.n_bytes ? (uint32_t)a.bits[B + j] : 0u);
        v = (v >> (24 - (int)(o & 7) - sc.bits)) & ((1u << sc.bits) - 1u);
        w[i >> 2] |= v << (8 * (i & 3));
    }
    return u4{w[0], w[1], w[2], w[3]};
}

// Per-element tx constellation indices of one symbol for this lane, from whichever
// source the launch uses: the lane generator's first 128 bits (philox mode) or the
// staged words (reference mode).  FB > 0: fixed b = FB, compile-time offsets.  In philox
// mode the generator g continues into the lane's noise (RX).  REF: the throughput kernel's lane
// block filled from the caller's bits instead (ref_lane; adaptive: ref_lane_adaptive).
template <int FB, int TPS, bool REF = false>
struct TxBits {
    u4 lane;
    Mwc64x g;
    const uint32_t* W;
    int base_bit;
    bool from_words;

    // payload words (P2, P3, m0, m1); the generator continues into the lane's noise
    __device__ __forceinline__ void seed_lane(uint64_t seed, int64_t s, int t) {
        const u4 p = philox_lane(seed, s, (uint32_t)t, kLane);
        g.seed(p.x, p.y);
        lane.x = p.z;
        lane.y = p.w;
        lane.z = g.next();
        lane.w = g.next();
    }
    __device__ __forceinline__ void load(const TxRxCommon& a, int64_t s, int t, uint32_t* Wslot, bool active) {
        from_words = FB == 0 && a.bits != nullptr;
        W = Wslot;
        base_bit = 0;
        lane.x = lane.y = lane.z = lane.w = 0u;
        if constexpr (REF && FB == 1) {
            if (active) lane = ref_lane_adaptive<TPS>(a, s, t);
        } else if constexpr (REF && FB > 1) {
            if (active) lane = ref_lane<FB, TPS>(a, s, t);
        } else if (from_words) {
            if (active) base_bit = stage_words<TPS>(a, s, Wslot, t);
        } else if (active) {
            seed_lane(a.seed, s, t);
        }
    }
    template <int I>
    __device__ __forceinline__ uint32_t fixed() const {
        return lane_bits(lane, I, FB);
    }
    // i: the element's index in the lane (philox mode); stream_off: its offset inside the
    // symbol's bit stream (reference mode)
    __device__ __forceinline__ uint32_t generic(int i, int b, int stream_off) const {
        if (from_words) return extract_w(W, base_bit + stream_off, b);
        return lane_bits(lane, i, b);
    }
};

// M-PSK as the reference builds it (constellation/models.py:356-380: LUT[gray(i)] =
// exp(2 pi j i / M)), complex64: the nearest point is the nearest angle, found without a
// search.  The point is folded into the first octant (|x|, |y|, swap when |y| > |x|), the
// sector inside the octant is counted against tan((q + 1/2) 2 pi / M) for q < M/8, and the
// three reflections are undone on the sector index k; the LUT index is gray(k).  M = 2 and
// 4 have no in-octant boundaries.  Decisions differ from the brute-force search only on a
// decision boundary (|y| = |x| or an exact tangent), a probability-zero event under noise.
template <typename R>
__device__ __forceinline__ uint32_t psk_decide(cpx<R> v, const TxRxCommon& cm) {
    const int M = cm.psk_m;
    const R ax = fabs(v.re), ay = fabs(v.im);
    const bool sw = ay > ax, sx = v.re < (R)0, sy = v.im < (R)0;
    const R u = fmax(ax, ay), w = fmin(ax, ay);  // angle of (u, w) in [0, pi/4]
    int k;
    if (M == 2) {
        k = sx ? 1 : 0;
    } else {
        int q = 0;
        for (int j = 0; j < (M >> 3); ++j) q += w > (sizeof(R) == 8 ? (R)cm.psk_tan64[j] : (R)cm.psk_tan[j]) * u;
        const int quarter = M >> 2;
        int k1 = sw ? quarter - q : q;        // reflect about 45 degrees
        if (M == 4) k1 = sw ? 1 : 0;
        int k2 = sx ? 2 * quarter - k1 : k1;  // reflect about 90 degrees
        k = sy ? (M - k2) & (M - 1) : k2;     // reflect about 0 degrees
    }
    return (uint32_t)(k ^ (k >> 1));
}

// Nearest constellation point of a non-separable LUT (PSK): the m points at offset off of the
// LUT pool (adaptive loading: the subcarrier's order; fixed: the whole single LUT).  complex128:
// the reference's |z - C_m| with hypot and the first index on ties (nn_index); complex64: the
// sector decision above for the reference's fixed M-PSK in throughput mode (cm.psk_m > 0 only
// there, ofdm_abi.hip fill_common), else squared distances in float against the plan-precision LUT.
template <typename R>
__device__ __forceinline__ uint32_t nn_decide(cpx<R> v, const TxRxCommon& cm, int off, int count) {
    if constexpr (sizeof(R) == 8) {
        return (uint32_t)nn_index(v.re, v.im, cm.lut64 + 2 * off, count);
    } else {
        if (cm.psk_m > 0) return psk_decide(v, cm);
        const cpx<float>* L = (const cpx<float>*)cm.lut + off;
        float bd = INFINITY;
        uint32_t best = 0;
        for (int m = 0; m < count; ++m) {
            const float dr = v.re - L[m].re, di = v.im - L[m].im;
            const float d = dr * dr + di * di;
            if (d < bd) {
                bd = d;
                best = (uint32_t)m;
            }
        }
        return best;
    }
}


// FFT of one symbol in a fused kernel: complex128 throughput kernels exchange through a row of
// reals (fft_reg_split), complex64 ones through the complex row with per-pass LDS twiddles, the
// generic kernel with the two-level table and recurrence.
template <typename R, int LOGN, bool INV, int FB>
__device__ __forceinline__ void fft_sym(cpx<R> (&x)[Geo<LOGN>::E], cpx<R>* row, const cpx<R>* tw,
                                        const cpx<R>* tt, int t) {
    if constexpr (split_rows<R, FB>())
        fft_reg_split<R, LOGN, INV, fast_tt<R, LOGN>()>(x, (R*)row, tw, tw + 64, t, tt);
    else
        fft_reg<R, LOGN, INV, (FB > 0)>(x, row, tw, tw + 64, t, tt);
}
// per-pass twiddle tables in LDS (throughput kernels while they fit) vs the two-level table
template <typename R, int LOGN, int FB>
constexpr bool uses_tt() { return FB > 0 && fast_tt<R, LOGN>(); }

// ============================================================ fused TX
// static (__shared__) LDS of k_tx beside its dynamic rows: the throughput kernels' LUT (2^FB
// entries; adaptive: the pool + a zero entry) and its two axis tables (tx_sep_lut)
template <int FB>
constexpr int tx_lut_static() { return FB == 1 ? kMaxLut + 1 : (FB > 1 ? (1 << FB) : 1); }
template <typename R, int FB, int LT>
constexpr int tx_sep_static() { return tx_sep_lut<R, FB, LT>() ? 2 * (1 << (FB / 2)) : 1; }
template <typename R, int FB, int LT>
constexpr size_t tx_static_lds() { return tx_lut_static<FB>() * sizeof(cpx<R>) + tx_sep_static<R, FB, LT>() * sizeof(R); }
// complex elements per symbol row: the plan's (tx_slot), or the window FIR's padded row if longer
template <typename R, int LOGN, int FB, int LT>
constexpr int tx_row_slot(int slot, int cp) {
    if (!(FB > 0 && LT > 0)) return slot;
    if (sizeof(R) == 8) {
        // complex128: the row of reals carries half a symbol's stream as complex samples, half 0's
        // m in [-(LT-1), cp + N/2) at wfir_in(A8 - cp + LT - 1 + m), and N / 2 transposed outputs
        const int A8 = (cp + 7) & ~7;
        slot = std::max(slot, 2 * (wfir_in(A8 + (1 << LOGN) / 2 + LT - 2, LT) + 1));
        return std::max(slot, 2 * (wfir_out((1 << LOGN) / 2 - 1) + 1));
    }
    // window FIR row: stream samples [-(LT-1), N+cp) at fir_pad(R0 + m)
    const int A = (cp + 15) & ~15, R0 = A - cp + LT - 1;
    return std::max(slot, fir_pad(R0 + (1 << LOGN) + cp) + 1);
}
// stream samples a symbol hands to the next one's FIR (the LDS keeps room for one without a channel)
constexpr int tx_tails(int L) { return L > 1 ? L - 1 : 1; }
// The dynamic LDS of k_tx at BLK threads for the plan's LUT length, staged bit words per symbol,
// FIR tail (tx_tails) and row slot: the kernel's layout and the launcher's byte count
template <typename R>
struct TxLds {
    cpx<R> *tw, *lut, *h, *hsw, *tails, *tt;
    AxisInfo* axis;
    unsigned char* rowmem;
    uint32_t *words, *sce;
    double* red;
    R* wlev;        // wide plan: the LUTs' scaled levels, kWideSide per LUT
    uint8_t* winv;  // wide plan: index bits -> level, [inv_i | inv_q] of kWideSide bytes per LUT
};
// n_wide (generic kernel): the LUTs of a plan with an order above 256, which maps from per-axis
// level tables (768 bytes per LUT in complex128) and stages no LUT -- lut_len is 0 then; a
// 4096-entry complex128 LUT alone would be 64 KB beside the N = 4096 symbol row's 68 KB
template <typename R, int LOGN, int FB, int LT, int BLK, typename CV>
__host__ __device__ __forceinline__ constexpr TxLds<R> tx_carve(CV& cv, int lut_len, int words_per_sym, int tls,
                                                                int slot, int n_wide = 0) {
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    // complex128 flat and window-FIR TX: a row of reals (fft_reg_split)
    // (the window FIR passes its stream through the row of reals twice: real, then imaginary parts)
    constexpr bool ROW_REAL = split_rows<R, FB>() && LT >= 0;
    constexpr bool TT = uses_tt<R, LOGN, FB>();
    TxLds<R> m{};
    m.tw = cv.template take<C>(TT ? 0 : 128);  // two-level twiddles (generic kernel, complex128 N > 1024)
    if constexpr (FB == 0) m.lut = cv.template take<C>(lut_len);  // (throughput kernels: static LDS)
    m.h = cv.template take<C>(32);
    m.hsw = cv.template take<C>(FB > 0 && LT > 0 ? 32 : 0);  // window FIR: the taps swizzled, (-im, re)
    m.axis = cv.template take<AxisInfo>(kMaxLuts);
    m.rowmem = cv.template take<unsigned char>((size_t)G::SPB * slot * (ROW_REAL ? sizeof(R) : sizeof(C)));
    m.tails = cv.template take<C>((size_t)G::SPB * tls);
    m.words = cv.template take<uint32_t>(FB ? 0 : (size_t)G::SPB * words_per_sym);  // reference bits
    m.red = cv.template take<double>(BLK / 64);
    m.tt = cv.template take<C>(TT ? tt_size(LOGN) : 0);  // throughput kernel: inverse per-pass twiddles
    // adaptive throughput kernel: per subcarrier (LUT offset << 8 | tx bit mask); unused
    // subcarriers point at a zero entry appended to the LUT pool
    m.sce = cv.template take<uint32_t>(FB == 1 ? G::N : 0);
    m.wlev = cv.template take<R>(FB == 0 ? (size_t)n_wide * kWideSide : 0);
    m.winv = cv.template take<uint8_t>(FB == 0 ? (size_t)n_wide * 2 * kWideSide : 0);
    return m;
}
// LT (throughput TX): 0 flat channel; 4 / 8 multipath with <= LT taps through the register
// window FIR (N >= 256, cp <= TPS); -1 any multipath (run-time loop over taps).  ZPW: the complex128
// window FIR with the zero-padding guard (and its run-time flat path for a one-tap channel) compiled
// in; without it (cyclic prefix, L > 1: the bench configs) the kernel needs ~139 VGPRs instead of
// 205-227 (3 waves per SIMD would fit with nothing spilled; measured no faster)
template <typename R, int FB, int LOGN, int LT, bool ZPW = false>
constexpr int tx_block() {
    if constexpr (sizeof(R) == 8 && FB > 0 && LT != 0) {
        // OFDM_F64_FIR_BLOCK threads if their LDS, static and dynamic, fits on the nominal channel
        // of these shapes (cp = 32, 8 taps)
        constexpr int BLK = OFDM_F64_FIR_BLOCK;
        CarveSize lds;
        tx_carve<R, LOGN, FB, LT, BLK>(lds, 0, 0, tx_tails(8), tx_row_slot<R, LOGN, FB, LT>(tx_slot(LOGN, 32, 8), 32));
        return lds.bytes + tx_static_lds<R, FB, LT>() <= kLdsPerCu ? BLK : 256;
    }
    if (sizeof(R) == 8 && FB > 0) return OFDM_F64_TX_BLOCK;
    return FB > 0 && LOGN <= 10 ? (LT != 0 ? OFDM_TX_MP_BLOCK : OFDM_TX_FAST_BLOCK) : kBlock;
}
constexpr int block_waves(int blk, int dflt) { return blk >= 512 ? 4 : dflt; }
template <typename R, int FB, int LOGN, int LT, bool ZPW = false>
constexpr int tx_waves() {
    if (sizeof(R) == 8 && FB > 0) {
        if (LT == 0) return OFDM_F64_TX_WAVES;
        return LOGN >= 12 ? OFDM_F64_FIR_WAVES_4K : OFDM_F64_FIR_WAVES;
    }
    if (FB > 0 && LT > 0 && LOGN > 10) return OFDM_TX_BIG_WFIR_WAVES;
    return block_waves(tx_block<R, FB, LOGN, LT>(), FB > 0 && LT > 0 ? OFDM_TX_WFIR_WAVES : OFDM_TX_WAVES);
}

// Each symbol group walks `chunk` consecutive OFDM symbols so the FIR tail (last L-1
// stream samples of the previous symbol) is carried in LDS; the first symbol of a chunk
// regenerates its predecessor's tail (one extra IFFT per chunk, L > 1 only).
// REF: the throughput kernel fed the caller's bits (reference streams, ref_lane) -- the same body
// WIDE: the generic kernel for a plan with an order above 256 (level tables instead of a staged
// LUT), an instantiation of its own so that the generic kernel of every other plan compiles as before
// CLIP: the soft limiter of ofdm_tx_clip (ofdm_hip.h: the definition) on the symbol in registers,
// directly after the IFFT: everything downstream -- prefix, FIR, tails, statistics -- sees the limited
// samples.  Instantiations of their own (ofdm_txclip_inst.hpp).  Invariant: the limiter's arguments are
// a separate trailing kernel parameter (Tail = TxClipTail) that only CLIP instantiations have; every
// other k_tx has an empty Tail, i.e. TxArgs alone, so its kernel-argument layout and code stay byte for
// byte what they were.  tx_tail(tail...) names that one parameter.
template <typename T>
__device__ __forceinline__ const T& tx_tail(const T& t) { return t; }
// The limiter's scale sqrt(A2 / p) for p > A2 > 0 as sa rsqrt(p), sa = sqrt(A2) once per kernel:
// complex64 v_rsq_f32 (1 ulp); complex128 v_rsq_f64 (~2^-26) and two Newton steps y += y e / 2,
// e = 1 - p y^2 (relative error ~1e-16 after the first; the second leaves ~1 ulp) -- 9 VALU against
// the ~45 of an IEEE division followed by an IEEE square root
template <typename R>
__device__ __forceinline__ R clip_scale(R sa, R p) {
    if constexpr (sizeof(R) == 4) {
        return sa * __builtin_amdgcn_rsqf(p);
    } else {
        R y = __builtin_amdgcn_rsq(p);
        y = __builtin_fma(y * (R)0.5, __builtin_fma(-(p * y), y, (R)1), y);
        y = __builtin_fma(y * (R)0.5, __builtin_fma(-(p * y), y, (R)1), y);
        return sa * y;
    }
}
template <typename R, int LOGN, int FB, int LT, bool ZPW = false, bool REF = false, bool WIDE = false,
          bool CLIP = false, typename... Tail>
__global__ __launch_bounds__((tx_block<R, FB, LOGN, LT, ZPW>()), (tx_waves<R, FB, LOGN, LT, ZPW>())) void k_tx(
    TxArgs a, Tail... tail) {
    static_assert(sizeof...(Tail) == (CLIP ? 1 : 0), "CLIP: one trailing TxClipTail; otherwise TxArgs alone");
    static_assert(!WIDE || (FB == 0 && LT == -1 && !REF), "the wide map lives in the generic kernel");
    static_assert(!CLIP || (!WIDE && !REF && !ZPW), "the limiter: the generic kernel and the Philox throughput forms");
    constexpr int BLK = tx_block<R, FB, LOGN, LT, ZPW>();
    constexpr bool WFIR = FB > 0 && LT > 0;  // register window FIR
    constexpr bool TX_NT = OFDM_TX_NT || (sizeof(R) == 8 && OFDM_TX_NT_F64);  // nontemporal y stores
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr int N = G::N, E = G::E, TPS = G::TPS;
    const TxRxCommon& cm = a.c;
    const int flags = ablation_flags(a.flags);
    const bool adaptive = FB ? false : (bool)cm.adaptive;
    // generic kernel variants: single-carrier OFDM (no IFFT, modulation/models.py:
    // 58-70) and the zero-padding guard (prefix/models.py:55-67: [x | 0 ... 0])
    const bool scm = FB == 1 ? false : (bool)cm.scm;  // SC-OFDM (run-time, uniform)
    // zero-padding guard (run-time, uniform); compiled out of the flat throughput TX (a zero
    // guard needs cp > 0, the launcher sends it to the LT = -1 kernel), where the run-time
    // row stride alone cost 15 % (config b TX 1.64 -> 1.92 ms)
    // (window FIR: only the ZPW instantiation -- the launcher sends zero padding there, and a one-tap
    // channel without it to the flat kernel, so the CP window FIR never takes the flat path below)
    constexpr bool ZP_OK = !(FB == 1 || (FB > 1 && LT == 0)) && (!WFIR || ZPW);
    constexpr bool FLAT_OK = !WFIR || ZPW;
    const bool zp = ZP_OK ? (bool)cm.zpad : false;
    const int ystride = ZP_OK ? cm.ystride : N;  // stored samples per OFDM symbol: N, or N + cp (ZP)
    const int cp = cm.cp, L = LT != 0 ? a.L : 1;
    const int slot = a.slot;  // complex elements per symbol row (>= PADN and >= L-1+cp+N)
    const int tls = L > 1 ? L - 1 : 1;  // tx_tails(L) spelled out (through the call the LT = -1 kernels compile differently)
    constexpr bool TT = uses_tt<R, LOGN, FB>();
    constexpr bool ROW_REAL = split_rows<R, FB>() && LT >= 0;  // (as tx_carve)
    // throughput kernels: the LUT in static LDS at a link-time address, so an element's LUT read
    // is addressed by its index bits alone; generic kernel: dynamic
    constexpr int LUT_STATIC = tx_lut_static<FB>();
    __shared__ C lut_s[LUT_STATIC];
    // complex128 multipath TX of square QAM: the LUT as its two axis tables (tx_sep_lut)
    constexpr bool SEP = tx_sep_lut<R, FB, LT>();
    constexpr int HB = FB / 2, SIDE = 1 << HB;
    __shared__ R sep_s[tx_sep_static<R, FB, LT>()];
    Carve cv(ofdm_smem);
    // a plan with an order above 256 (WIDE): level tables instead of a staged LUT
    const int n_wide = WIDE ? cm.n_axis : 0;
    const TxLds<R> lds = tx_carve<R, LOGN, FB, LT, BLK>(cv, cm.lut_len, cm.words_per_sym, tls, slot, n_wide);
    C *tw = lds.tw, *lut = FB > 0 ? lut_s : lds.lut, *h = lds.h, *hsw = lds.hsw, *tails = lds.tails, *tt = lds.tt;
    AxisInfo* axis = lds.axis;
    unsigned char* rowmem = lds.rowmem;
    uint32_t *words = lds.words, *sce = lds.sce;
    double* red = lds.red;
    constexpr int TTS = TT ? tt_size(LOGN) : 0;

    // the tables' global reads issued first (Staged), then the LDS writes
    constexpr bool FOLD_H0 = FB > 0 && LT == 0;
    const C* glut = (const C*)cm.lut;
    Staged<BLK, TTS, C> st_tt;
    Staged<BLK, (FB > 0 ? LUT_STATIC : BLK), C, (FB > 0)> st_lut;  // (generic kernel: any LUT length)
    Staged<BLK, (FB == 1 ? N : 0), ScInfo> st_sc;
    Staged<BLK, kMaxLuts, Dwords<AxisInfo>> st_ax;
    static_assert(kMaxLuts <= BLK && 32 <= BLK, "one axis entry / tap per thread");
    C hq = mk<R>(0, 0), sep_a = mk<R>(0, 0), sep_b = mk<R>(0, 0), hf = mk<R>(1, 0);
    int ax_off = 0;
    if constexpr (FOLD_H0) hf = ((const C*)a.h)[0];
    st_tt.load((const C*)cm.ptw + TTS, TTS);
    st_lut.load(glut, cm.lut_len);
    if constexpr (FB == 1) st_sc.load(cm.sc, N);
    st_ax.load((const Dwords<AxisInfo>*)cm.axis, cm.n_axis);
    if (threadIdx.x < L && threadIdx.x < 32) hq = ((const C*)a.h)[threadIdx.x];
    // adaptive: lane l of every wave holds order l's LUT offset, for the codes' lane shuffle
    if constexpr (FB == 1) {
        if ((int)(threadIdx.x & 63) < cm.n_axis) ax_off = cm.axis[threadIdx.x & 63].lut_off;
    }
    if constexpr (SEP) {
        if (threadIdx.x < SIDE) sep_a = glut[threadIdx.x], sep_b = glut[threadIdx.x << HB];
    }
    if constexpr (!TT) load_twiddles<R>(tw, (const C*)cm.tw);
    // the 1/sqrt(N) of ifft(norm="ortho") folded into the LUT (same product per element);
    // flat throughput kernel: the channel tap too (y = h0 ifft(X) = ifft(h0 X)), so the
    // symbol leaves the IFFT as the channel output
    const R lut_scale = scm ? (R)1 : (R)cm.scale;
    st_tt.store(tt);
    st_lut.store(lut, [&](const C& v) { return cscale(FOLD_H0 ? cmul(hf, v) : v, lut_scale); });
    if constexpr (SEP) {
        // LUT[i] = I[i & (SIDE - 1)] + j Q[i >> HB] exactly (the plan's build_axis verified it):
        // I from the entries with Q index 0, Q from those with I index 0, the same scaled values
        if (threadIdx.x < SIDE) {
            sep_s[threadIdx.x] = sep_a.re * lut_scale;
            sep_s[SIDE + threadIdx.x] = sep_b.im * lut_scale;
        }
    }
    st_ax.store((Dwords<AxisInfo>*)axis);
    if constexpr (WIDE) {
        // wide plan: each LUT's levels with the 1/sqrt(N) folded in -- the staged LUT's single
        // multiply per component, on the same values (LUT[i] = lev[ki] + j lev[kq] exactly, and the
        // plan-precision LUT is the rounded double one) -- and its index -> level maps
        for (int i = threadIdx.x; i < n_wide * kWideSide; i += BLK) {
            const int l = i / kWideSide, k = i % kWideSide;
            const WideAxis& wa = a.wide[l];
            lds.wlev[i] = (R)wa.lev[k] * lut_scale;
            lds.winv[2 * kWideSide * l + k] = wa.inv_i[k];
            lds.winv[2 * kWideSide * l + kWideSide + k] = wa.inv_q[k];
        }
    }
    if constexpr (FB == 1) {
        if (threadIdx.x == 0) lut[cm.lut_len] = mk<R>(0, 0);
        auto code = [&](const ScInfo& sc, int off) {
            return sc.lut < 0 ? (uint32_t)cm.lut_len << 8 : ((uint32_t)off << 8) | ((1u << sc.bits) - 1u);
        };
        // the order's LUT offset from the lane holding it (a dependent global read per element
        // had been waited for one by one); entries past the staged ones (N > 8 BLK) read directly
        int k0 = threadIdx.x;
#pragma unroll
        for (int q = 0; q < st_sc.K; ++q, k0 += BLK) {
            const ScInfo sc = st_sc.v[q];
            // (a slot past N was never loaded: its lane index is taken as 0, not read)
            const int lid = k0 < N ? (int)sc.lut : -1;
            const int off = __shfl(ax_off, lid < 0 ? 0 : lid);
            if (k0 < N) sce[k0] = code(sc, off);
        }
        for (int k = k0; k < N; k += BLK) {
            const ScInfo sc = cm.sc[k];
            sce[k] = code(sc, sc.lut < 0 ? 0 : cm.axis[sc.lut].lut_off);
        }
    }
    if (threadIdx.x < 32) {
        h[threadIdx.x] = hq;
        if (WFIR) hsw[threadIdx.x] = mk<R>(-hq.im, hq.re);  // window FIR (complex64): taps swizzled
    }
    __syncthreads();

    const int ls = TPS >= 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x / TPS) : threadIdx.x / TPS;
    const int t = threadIdx.x % TPS;
    C* row = (C*)(rowmem + (size_t)ls * slot * (ROW_REAL ? sizeof(R) : sizeof(C)));
    C* tl = tails + ls * tls;
    uint32_t* W = words + ls * cm.words_per_sym;
    C* yout = (C*)a.y;
    const C h0 = h[0];
    // window FIR: the stream sample m in [-(LT-1), N+cp) lives at row[fir_pad(R0 + m)], R0 chosen
    // so that lane t's window (samples cp + 16 t - (LT-1) ..) starts at row index A + 16 t,
    // A = 16 ceil(cp/16)
    constexpr int LTN = WFIR ? LT : 1;
    const int A = (cp + 15) & ~15, R0 = A - cp + LTN - 1;
    const int64_t ngroups = (cm.n_sym + a.chunk - 1) / a.chunk;
    const int64_t niter = (ngroups + G::SPB - 1) / G::SPB;
    // sum |y|^2 in exact fixed point (fx_accum, per lane and symbol); |x|^2 statistics in double
    unsigned long long pq0 = 0, pq1 = 0;
    double px = 0, mx = 0;
    // CLIP: the threshold on |x|^2 and sqrt of it in the plan's precision; the lane's samples over the
    // threshold and samples examined, of the call's own symbols (active, c >= 0) only
    [[maybe_unused]] R clip_a2 = 0, clip_sa = 0;
    [[maybe_unused]] uint32_t n_clip = 0, n_seen = 0;
    if constexpr (CLIP) {
        clip_a2 = (R)tx_tail(tail...).a2;
        clip_sa = sqrt(clip_a2);
    }

    for (int64_t it = blockIdx.x; it < niter; it += gridDim.x) {
        const int64_t grp = it * G::SPB + ls;
        const int64_t sbeg = grp * a.chunk;  // local symbol index
        for (int c = (L > 1 ? -1 : 0); c < a.chunk; ++c) {
            const int64_t sl = sbeg + c;
            const int64_t sg = cm.sym0 + sl;
            const bool active = grp < ngroups && sl < cm.n_sym && sg >= 0;
            TxBits<FB, TPS, REF> tb;
            tb.load(cm, sg, t, W, active && !(flags & 1));
            if (FB == 0) sym_sync<TPS>();  // staged words visible
            // map (QAMConstellationMapper.encode, constellation/models.py:240-246); the
            // 1/sqrt(N) of ifft(norm="ortho") folded in
            // (throughput kernels: an inactive symbol maps its zero lane words -- nothing of it
            // is stored or counted, and its tail is zeroed below)
            C x[E];
            if constexpr (FB == 1) {
                // element i: the low b_k bits of lane byte i through its subcarrier's LUT.  The
                // table index is made opaque per symbol so the 16 loop-invariant reads are not
                // hoisted out of the symbol loop as 16 live registers.
                int st = t;
                asm volatile("" : "+v"(st));
                static_for<0, E>([&](auto I) {
                    const uint32_t e = sce[st + I * TPS];
                    const uint32_t v = (lane_word(tb.lane, I >> 2) >> (8 * (I & 3))) & e & 0xFFu;
                    x[I] = lut[(e >> 8) + v];
                });
            } else if (SEP && cm.psk_m == 0) {
                // two 8-byte reads from SIDE-entry tables: distinct entries sit on distinct banks
                // (the 2^FB-entry complex table's random 16-byte reads conflicted); the reference's
                // 4/16-PSK (not separable) take the complex table below
                static_for<0, E>([&](auto I) {
                    const uint32_t v = tb.template fixed<I>();
                    x[I] = mk<R>(sep_s[v & (SIDE - 1)], sep_s[SIDE + (v >> HB)]);
                });
            } else if constexpr (FB > 0) {
                static_for<0, E>([&](auto I) { x[I] = lut[tb.template fixed<I>()]; });
            } else if constexpr (WIDE) {
                // a plan with an order above 256: every LUT of it maps through its
                // level tables, x = lev[inv_i[idx & (side - 1)]] + j lev[inv_q[idx >> hbits]] -- the
                // LUT entry's own components, scaled as the staged LUT would be; a non-separable
                // LUT (PSK) is read from the plan's table in global memory
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const int k = t + i * TPS;
                    C v = mk<R>(0, 0);
                    int lid = 0, b = cm.b, off = k * cm.b;
                    if (adaptive) {
                        const ScInfo sc = cm.sc[k];
                        lid = sc.lut;
                        b = sc.bits;
                        off = sc.bitoff;
                    }
                    if (active && lid >= 0) {
                        const uint32_t idx = tb.generic(i, b, off);
                        const AxisInfo& ax = axis[lid];
                        if (cm.nn) {
                            v = cscale(glut[ax.lut_off + idx], lut_scale);
                        } else {
                            const uint8_t* inv = lds.winv + 2 * kWideSide * lid;
                            const R* lev = lds.wlev + kWideSide * lid;
                            v = mk<R>(lev[inv[idx & (uint32_t)(ax.side - 1)]], lev[inv[kWideSide + (idx >> ax.hbits)]]);
                        }
                    }
                    x[i] = v;
                }
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
            if (!(flags & 2) && !scm) fft_sym<R, LOGN, true, FB>(x, row, tw, tt, t);
            // CLIP: x' = x sqrt(A2 / p) where p = |x|^2 > A2 -- every symbol that feeds the stream, the
            // regenerated predecessor (c < 0) too; only the call's own symbols are counted.  The
            // limited samples' |x'|^2, its sum and maximum (in the order of the statistics below,
            // which take them from here) are formed in the same pass.
            [[maybe_unused]] R clip_sum = 0, clip_max = 0;
            if constexpr (CLIP) {
                uint32_t nc = 0;
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    R p2 = norm2(x[i]);
                    if (p2 > clip_a2) {
                        x[i] = cscale(x[i], clip_scale<R>(clip_sa, p2));
                        p2 = norm2(x[i]);
                        ++nc;
                    }
                    clip_sum += p2;
                    clip_max = fmax(clip_max, p2);
                }
                if (active && c >= 0) {
                    n_clip += nc;
                    n_seen += E;
                }
            }
            // The prefix repeats samples k >= N - cp.  With cp <= TPS only the lane's last
            // element can be one of them (one loop-invariant compare); otherwise the compares
            // are made per symbol against an opaque copy of N - cp, so they are not hoisted
            // as E live 64-bit masks (SGPR spills).
            int ncp = N - cp;
            asm volatile("" : "+s"(ncp));
            auto prefix_sum = [&](auto&& pw) -> R {
                if (zp) return (R)0;  // the zero guard adds no power
                if (WFIR || cp <= TPS) return t >= TPS - cp ? pw(E - 1) : (R)0;  // (window FIR: cp <= TPS)
                R acc = 0;
#pragma unroll
                for (int i = 0; i < E; ++i)
                    if (t + i * TPS >= ncp) acc += pw(i);
                return acc;
            };
            // PAPR statistics over the modulated symbol incl. its prefix (simulation/models.py:519-522)
            R pxs = 0;
            if (active && c >= 0) {
                R mxs = 0;  // per-symbol partials in the arithmetic precision
                if constexpr (CLIP) {
                    pxs = clip_sum;
                    mxs = clip_max;
                } else {
#pragma unroll
                    for (int i = 0; i < E; ++i) {
                        const R p2 = norm2(x[i]);
                        pxs += p2;
                        // (complex128 flat channel: v_max_f64 directly, 15 VALU per symbol and lane fewer;
                        // the window-FIR kernels schedule fmax without the quieting step already, and the
                        // complex64 ones grow with it)
                        mxs = (sizeof(R) == 8 && LT == 0) ? peak_max(mxs, p2) : fmax(mxs, p2);
                    }
                }
                pxs += prefix_sum([&](int i) { return norm2(x[i]); });
                px += pxs;
                mx = fmax(mx, (double)mxs);
            }
            if (FLAT_OK && L == 1) {
                // flat channel: y = h0 x, no inter-symbol memory
                if (active && c >= 0) {
                    C* yo = yout + sl * ystride;
#pragma unroll
                    for (int i = 0; i < E; ++i) {
                        const C yv = FOLD_H0 ? x[i] : cmul(h0, x[i]);
                        if (!yout || (flags & 4)) continue;
                        if constexpr (FB > 0 && TPS >= 64) {
                            // the row base is wave-uniform: made explicit, the stores take the
                            // SGPR-base + 32-bit lane-offset form instead of a loop-carried 64-bit
                            // VGPR pointer (which spilled to scratch, and whose per-symbol reload's
                            // vmcnt(0) waited for all of the previous symbol's stores)
                            st_stream<TX_NT>(lane_ptr(uniform_ptr(yo), (uint32_t)(t + i * TPS)), yv);
                        } else {
                            st_stream<(FB > 0 && TX_NT)>(yo + t + i * TPS, yv);
                        }
                    }
                    if (zp && yout)
                        for (int j = t; j < cp; j += TPS) yo[N + j] = mk<R>(0, 0);
                    if constexpr (FOLD_H0) {
                        fx_accum((R)pxs, pq0, pq1);  // the statistics above were taken on y (x |h0|^2 fixed below)
                    } else if constexpr (FB > 0) {
                        fx_accum((R)(norm2(h0) * pxs), pq0, pq1);  // |y|^2 = |h0|^2 |x|^2 (complex64 mode)
                    } else {
                        R pys = 0;
#pragma unroll
                        for (int i = 0; i < E; ++i) pys += norm2(cmul(h0, x[i]));
                        pys += prefix_sum([&](int i) { return norm2(cmul(h0, x[i])); });
                        fx_accum((R)pys, pq0, pq1);
                    }
                }
                sym_sync<TPS>();  // W / row reuse by the next symbol
            } else if constexpr (WFIR) {
                // throughput multipath (L <= LT, cp <= TPS, E = 16, TPS >= 16): lane t computes the
                // 16 consecutive kept samples k = 16 t + j from a register window of 16 + LT - 1
                // stream samples read once from LDS (fir_pad: lane stride 17 elements, conflict
                // free; offsets compile-time) -- 23 LDS reads instead of 2 L per output
                static_assert(E == 16 && TPS >= 16, "window FIR geometry");
                constexpr int WN = E + LT - 1;
                if constexpr (sizeof(R) == 8) {
                    // complex128: the FIR runs over the symbol in two halves of N / 2 kept samples,
                    // through the symbol's row of reals used as complex samples, one pad slot per 8
                    // (wfir_in).  Half h holds the stream samples m in [cp + h N/2 - (LT-1),
                    // cp + (h+1) N/2) at wfir_in(B_h + m) -- half 0 from m = -(LT-1): the previous
                    // symbol's tail and the prefix region too -- and lane t computes the 8
                    // consecutive kept samples k = h N/2 + 8 t + j from a window of 8 + LT - 1
                    // complex samples (ds_read_b128 at lane stride 9: conflict free), streamed one
                    // sample at a time through the outputs' accumulators in Gauss's three-
                    // multiplication form:
                    //   T = sum hr (wr + wi),  U = sum (hr + hi) wi,  V = sum (hi - hr) wr,
                    //   y = (T - U, T + V)
                    // (3 v_fma_f64 per tap and output; the taps' three forms in scalar registers,
                    // TxArgs::gtap, zero past L).  Live at once: half a symbol's elements, 24
                    // accumulators and the streamed sample -- against two whole windows of reals and
                    // 16 outputs' sums when the row carried the real and then the imaginary parts.
                    // The outputs leave through the row (kk = 8 t + j at wfir_out(kk), read back as
                    // kk = t + TPS i) and buffer stores: lanes 8 m .. 8 m + 7 store one whole
                    // 128-byte line.
                    // Zero padding (prefix/models.py:55-67, the stream [x | 0 ... 0]): x starts at
                    // stream sample 0 instead of cp, every one of the N + cp outputs is stored
                    // (ystride N + cp: the receiver overlap-adds the guard), the guard outputs
                    // N + t (t < cp) from the last LT - 1 samples of x in half 1's row, and the
                    // tail for the next symbol from that row too (the stream ends in the guard).
                    static_assert(LT <= kWinTaps, "window FIR taps");
                    constexpr int WH = 8 + LT - 1;
                    C* crow = (C*)row;
                    // (a complex sample as one ds_write_b128: as two ds_write_b64 -- 12 LDS cycles per KB
                    // against 13 -- TX e ran 4.78 -> 5.02 ms, profiles/r04m_ab_fir_write_b64.txt)
                    auto st16 = [&](int slot_, C v) { *(f64x2*)(crow + slot_) = f64x2{v.re, v.im}; };
                    auto ld16 = [&](const C* p) { const f64x2 u = *(const f64x2*)p; return mk<R>(u.x, u.y); };
                    const bool live = active && c >= 0;
                    const bool store = live && yout && !(flags & 4);
                    R hr[LT], c1[LT], c2[LT];
#pragma unroll
                    for (int q = 0; q < LT; ++q) {
                        hr[q] = a.gtap[0][q];
                        c1[q] = a.gtap[1][q];
                        c2[q] = a.gtap[2][q];
                    }
                    // LDS offsets and lane conditions from opaque per-symbol copies of t, cp and L,
                    // each offset a per-symbol base plus compile-time constants: hoisted out of the
                    // symbol loop they were ~20 loop-invariant registers, spilled to scratch
                    int to = t, cpo = cp, lo = L;
                    asm volatile("" : "+v"(to), "+s"(cpo), "+s"(lo));
                    if (c < 0 && !zp) {
                        // a group's regenerated predecessor: only its tail is needed, the last
                        // L - 1 samples of x (registers); no FIR, no stores
                        sym_sync<TPS>();  // the previous symbol's FIR has read the old tail
                        if (to >= TPS - (lo - 1)) tl[to - (TPS - (lo - 1))] = active ? x[E - 1] : mk<R>(0, 0);
                        sym_sync<TPS>();
                        continue;
                    }
                    const int so = zp ? 0 : cpo;  // stream sample of x[0]
                    const int A8 = (so + 7) & ~7;
                    R pys = 0;
                    static_for<0, 2>([&](auto HH) {
                        constexpr int h = HH;
                        constexpr int NH = N / 2;
                        // stream sample m at wfir_in(B + m); the lanes' windows start at Ah + 8 t
                        const int Ah = h == 0 ? A8 : 0;
                        const int B = Ah - so - h * NH + (LT - 1);
                        sym_sync<TPS>();  // the FFT's last pass / the previous half's stores have read the row
                        // this half's elements: kept k = t + TPS i (stream cp + k) for k in
                        // [h N/2 - (LT-1), (h+1) N/2); TPS i = N/2 at i = 8
                        // (TPS i = 0 mod 8: wfir_in(b + TPS i) = wfir_in(b) + 9 TPS i / 8)
                        const int bx = wfir_in(B + so + to, LT);
                        static_for<0, E>([&](auto I) {
                            constexpr int i = I;
                            constexpr int off = 9 * TPS * i / 8;
                            if constexpr (i >= 8 * h && i < 8 * h + 8) {
                                st16(bx + off, x[i]);
                            } else if constexpr (h == 1 && i == 7) {
                                if (to >= TPS - (LT - 1)) st16(bx + off, x[i]);
                            }
                        });
                        if constexpr (h == 0) {
                            if (!zp && to >= TPS - cpo) st16(wfir_in(B + to - (TPS - cpo), LT), x[E - 1]);  // cyclic prefix
                            if (to < LT - 1) {  // stream samples -(LT-1) .. -1: zeros, then the previous tail
                                const int z = to - (LT - lo);
                                st16(wfir_in(B - (LT - 1) + to, LT), z < 0 ? mk<R>(0, 0) : tl[z]);
                            }
                        }
                        sym_sync<TPS>();
                        if constexpr (h == 0) {
                            // this symbol's tail for the next one, from the registers (the old tail
                            // has been copied): its last L - 1 stream samples, lanes TPS - (L-1) ..
                            if (!zp && to >= TPS - (lo - 1)) tl[to - (TPS - (lo - 1))] = active ? x[E - 1] : mk<R>(0, 0);
                        } else {
                            // zero padding: the last L - 1 stream samples N + cp - (L-1) + z are x
                            // below N, guard zeros from N on
                            if (zp && to < lo - 1) {
                                const int m = N + cpo - (lo - 1) + to;
                                tl[to] = (active && m < N) ? ld16(crow + wfir_in(B + m, LT)) : mk<R>(0, 0);
                            }
                        }
                        // every lane streams its window, live or not (under the live condition the
                        // accumulators would be conditionally defined and spill)
                        // (wfir_in(Ah + 8 t + W) = wfir_in(Ah) + 9 t + W + (W + ioff) / 8)
                        constexpr int IOFF = wfir_ioff(LT);
                        R T[8], U[8], V[8];
                        // the window read two samples ahead of its use, in program order (the compiler
                        // issues all 8 + LT - 1 reads at once either way; tying each read to the previous
                        // sample's sums through an empty asm ran 1 % slower)
                        typedef const __attribute__((address_space(3))) f64x2* lwin;
                        lwin wl = (lwin)(crow + (wfir_in(Ah, LT) + 9 * to));
                        auto ldw = [&](int k) { const f64x2 u = wl[k]; return mk<R>(u.x, u.y); };
                        C ring[3];
                        ring[0] = ldw(IOFF >> 3);
                        ring[1] = ldw(1 + ((1 + IOFF) >> 3));
                        static_for<0, WH>([&](auto W) {
                            const C e = ring[W % 3];
                            const R sw = e.re + e.im;
                            if constexpr (W + 2 < WH) {
                                ring[(W + 2) % 3] = ldw((W + 2) + ((W + 2 + IOFF) >> 3));
                            }
                            static_for<0, LT>([&](auto Q) {  // tap Q of output j
                                constexpr int j = W - (LT - 1) + Q;
                                if constexpr (j >= 0 && j < 8) {
                                    if constexpr (Q == LT - 1) {  // the output's first term
                                        T[j] = hr[Q] * sw;
                                        U[j] = c1[Q] * e.im;
                                        V[j] = c2[Q] * e.re;
                                    } else {
                                        T[j] = __builtin_fma(hr[Q], sw, T[j]);
                                        U[j] = __builtin_fma(c1[Q], e.im, U[j]);
                                        V[j] = __builtin_fma(c2[Q], e.re, V[j]);
                                    }
                                }
                            });
                            __builtin_amdgcn_sched_barrier(0);
                        });
                        if constexpr (h == 1) {
                            // zero padding: guard output N + t = sum over l > t of h_l x[N + t - l]
                            // (the guard's own samples are zero), stored and counted
                            if (zp && live && to < cpo) {
                                R pT = 0, pU = 0, pV = 0;
#pragma unroll
                                for (int l = 1; l < LT; ++l) {
                                    if (l <= to) continue;
                                    const C e = ld16(crow + wfir_in(B + N + to - l, LT));
                                    pT = __builtin_fma(hr[l], e.re + e.im, pT);
                                    pU = __builtin_fma(c1[l], e.im, pU);
                                    pV = __builtin_fma(c2[l], e.re, pV);
                                }
                                const C yv = mk<R>(pT - pU, pT + pV);
                                pys = __builtin_fma(yv.re, yv.re, pys);
                                pys = __builtin_fma(yv.im, yv.im, pys);
                                if (store) yout[sl * ystride + N + to] = yv;
                            }
                        }
                        if constexpr (h == 0) {
                            if (!zp && live && to < cpo) {  // prefix-region output m = t: power only (noise/models.py:14)
                                R pT = 0, pU = 0, pV = 0;
#pragma unroll
                                for (int l = 0; l < LT; ++l) {
                                    const C e = ld16(crow + wfir_in(B + to - l, LT));
                                    pT = __builtin_fma(hr[l], e.re + e.im, pT);
                                    pU = __builtin_fma(c1[l], e.im, pU);
                                    pV = __builtin_fma(c2[l], e.re, pV);
                                }
                                const R pr = pT - pU, pi = pT + pV;
                                pys = __builtin_fma(pr, pr, pys);
                                pys = __builtin_fma(pi, pi, pys);
                            }
                        }
                        sym_sync<TPS>();  // every window is read: the outputs take the row
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const C yv = mk<R>(T[j] - U[j], T[j] + V[j]);
                            pys = __builtin_fma(yv.re, yv.re, pys);
                            pys = __builtin_fma(yv.im, yv.im, pys);
                            st16(8 * to + (j ^ (to & 7)), yv);  // wfir_out(8 t + j)
                        }
                        sym_sync<TPS>();
                        if (store) {
                            // global stores off two wave-uniform bases (elements i < 4 and i >= 4),
                            // the lane's 32-bit byte offset in one VGPR and element i's in the
                            // instruction's offset field (per-element 64-bit VGPR addresses were
                            // loop-invariant registers).  (Buffer stores with SGPR offsets here
                            // corrupted the last store's low data dword on gfx950: the compiler
                            // inserts no wait state between such a store and a VALU write of its
                            // data VGPRs.)
                            C* yh = yout + sl * ystride + h * NH;
                            const C* rb = crow + wfir_out(to);
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                // (TPS = 0 mod 64: wfir_out(t + TPS i) = wfir_out(t) + TPS i)
                                const C* ri = TPS % 64 == 0 ? rb + TPS * i : crow + wfir_out(to + TPS * i);
                                if constexpr (TPS >= 64) {
                                    gptr<C> yg = uniform_ptr(yh + (i >> 2) * 4 * TPS);
                                    st_stream<TX_NT>(lane_ptr(yg, (uint32_t)to) + (i & 3) * TPS, ld16(ri));
                                } else {
                                    st_stream<TX_NT>((gptr<C>)yh + to + TPS * i, ld16(ri));
                                }
                            }
                        }
                    });
                    if (live) fx_accum((R)pys, pq0, pq1);
                    sym_sync<TPS>();
                } else {
                    sym_sync<TPS>();  // the last FFT pass has read the row
                    {
                        const int u = R0 + cp + t;  // stream sample cp + t + TPS i at fir_pad(u + TPS i)
                        const int bx = fir_pad(u);
#pragma unroll
                        for (int i = 0; i < E; ++i) row[bx + TPS * i + (TPS * i >> 4)] = x[i];  // TPS i = 0 mod 16
                    }
                    if (t >= TPS - cp) row[fir_pad(R0 + t - (TPS - cp))] = x[E - 1];  // cyclic prefix
                    if (t < LT - 1) {  // stream samples -(LT-1) .. -1: zeros, then the previous tail
                        const int z = t - (LT - L);
                        row[fir_pad(R0 - (LT - 1) + t)] = z < 0 ? mk<R>(0, 0) : tl[z];
                    }
                    sym_sync<TPS>();
                    // complex64: taps (zero past L), LDS broadcast reads; the opaque offset keeps
                    // the reads in the symbol loop (hoisted, the 4 LT registers stay live through
                    // the FFT and spill)
                    const bool live = active && c >= 0;
                    int ho = 0;
                    asm volatile("" : "+v"(ho));
                    f32x2 hv[LT], hs[LT];
#pragma unroll
                    for (int q = 0; q < LT; ++q) {
                        hv[q] = f32x2{(float)h[ho + q].re, (float)h[ho + q].im};
                        hs[q] = f32x2{(float)hsw[ho + q].re, (float)hsw[ho + q].im};
                    }
                    // the window (every lane, live or not), the prefix-region output and the tail
                    // leave the row first: the outputs take its place
                    const C* wb = row + (A + (A >> 4) + 17 * t);
                    f32x2 win[WN];
#pragma unroll
                    for (int w = 0; w < WN; ++w) {
                        const C ev = wb[w + (w >> 4)];
                        win[w] = f32x2{(float)ev.re, (float)ev.im};
                    }
                    R pys = 0;
                    if (live && t < cp) {  // prefix-region outputs: power only (noise/models.py:14)
                        f32x2 yp = f32x2{0.f, 0.f};
#pragma unroll
                        for (int l = 0; l < LT; ++l) {
                            const C ev = row[fir_pad(R0 + t - l)];
                            const f32x2 e = f32x2{(float)ev.re, (float)ev.im};
                            yp = __builtin_elementwise_fma(e.xx, hv[l], yp);
                            yp = __builtin_elementwise_fma(e.yy, hs[l], yp);
                        }
                        pys = yp.x * yp.x + yp.y * yp.y;
                    }
                    // tail for the next symbol: the last L-1 stream samples (zeros before symbol 0)
                    if (t < L - 1) tl[t] = active ? row[fir_pad(R0 + N + cp - (L - 1) + t)] : mk<R>(0, 0);
                    sym_sync<TPS>();
                    // the lane's 16 consecutive outputs k = 16 t + j go to row[fir_pad(k)] and
                    // leave as k = t + TPS i: whole-line stores instead of 16 lines per lane
                    f32x2 pacc = f32x2{0.f, 0.f};  // (sum Re^2, sum Im^2): one packed FMA per output
#pragma unroll
                    for (int j = 0; j < E; j += 2) {
                        f32x2 y0 = f32x2{0.f, 0.f}, y1 = f32x2{0.f, 0.f};
#pragma unroll
                        for (int l = 0; l < LT; ++l) {
                            const f32x2 e0 = win[j + LT - 1 - l], e1 = win[j + LT - l];
                            y0 = __builtin_elementwise_fma(e0.xx, hv[l], y0);
                            y0 = __builtin_elementwise_fma(e0.yy, hs[l], y0);
                            y1 = __builtin_elementwise_fma(e1.xx, hv[l], y1);
                            y1 = __builtin_elementwise_fma(e1.yy, hs[l], y1);
                        }
                        pacc = __builtin_elementwise_fma(y0, y0, pacc);
                        pacc = __builtin_elementwise_fma(y1, y1, pacc);
                        row[fir_pad(E * t + j)] = mk<R>(y0.x, y0.y);
                        row[fir_pad(E * t + j + 1)] = mk<R>(y1.x, y1.y);
                    }
                    sym_sync<TPS>();
                    if (live && yout && !(flags & 4)) {
                        C* ys = yout + sl * N;
                        int to = t;  // opaque: offsets hoisted out of the loop would hold registers
                        asm volatile("" : "+v"(to));
                        gptr<C> yg = TPS >= 64 ? uniform_ptr(ys) : (gptr<C>)ys;
#pragma unroll
                        for (int i = 0; i < E; ++i)
                            st_stream<TX_NT>(lane_ptr(yg, (uint32_t)(to + TPS * i)), row[fir_pad(to + TPS * i)]);
                    }
                    if (live) fx_accum((R)(pys + pacc.x + pacc.y), pq0, pq1);
                    sym_sync<TPS>();
                }
            } else {
                // extended serial stream in the row: [tail (L-1) | prefix (cp) | x (N)], or with
                // zero padding [tail (L-1) | x (N) | zeros (cp)]
                sym_sync<TPS>();  // the last FFT pass has read the row
                const int o = zp ? L - 1 : L - 1 + cp;
#pragma unroll
                for (int i = 0; i < E; ++i) row[o + t + i * TPS] = x[i];
                if (zp) {
                    for (int j = t; j < cp; j += TPS) row[L - 1 + N + j] = mk<R>(0, 0);
                } else if (cp <= TPS) {
                    if (t >= TPS - cp) row[L - 1 + t - (TPS - cp)] = x[E - 1];
                } else {
#pragma unroll
                    for (int i = 0; i < E; ++i) {
                        const int k = t + i * TPS;
                        if (k >= ncp) row[L - 1 + k - ncp] = x[i];
                    }
                }
                for (int j = t; j < L - 1; j += TPS) row[j] = tl[j];
                sym_sync<TPS>();
                if (active && c >= 0) {
                    // linear convolution with the unit-power CIR (channel/models.py:52-55)
                    R pys = 0;
                    for (int m = t; m < N + cp; m += TPS) {
                        C yv = mk<R>(0, 0);
                        const C* e = row + (L - 1 + m);
#pragma unroll 8
                        for (int l = 0; l < L; ++l) yv = yv + cmul(h[l], e[-l]);
                        pys += norm2(yv);
                        if (yout && !(flags & 4)) {
                            if (zp)
                                yout[sl * ystride + m] = yv;  // every stream sample (RX overlap-adds)
                            else if (m >= cp)
                                yout[sl * N + (m - cp)] = yv;
                        }
                    }
                    fx_accum((R)pys, pq0, pq1);
                }
                // tail for the next symbol: the last L-1 stream samples (zeros before symbol 0)
                for (int j = t; j < L - 1; j += TPS) tl[j] = active ? row[N + cp + j] : mk<R>(0, 0);
                sym_sync<TPS>();
            }
        }
    }
    if constexpr (FOLD_H0) {  // |x|^2 = |y|^2 / |h0|^2
        const double ih2 = 1.0 / ((double)h0.re * (double)h0.re + (double)h0.im * (double)h0.im);
        px *= ih2;
        mx *= ih2;
    }
    fx_normalize(pq0, pq1);
    pq0 = block_sum<unsigned long long, BLK>(pq0, (unsigned long long*)red);
    pq1 = block_sum<unsigned long long, BLK>(pq1, (unsigned long long*)red);
    px = block_sum<double, BLK>(px, red);
    mx = block_max<double, BLK>(mx, red);
    if (threadIdx.x == 0) {
        unsigned long long* pr = (unsigned long long*)a.partials + (size_t)blockIdx.x * kTxFields;
        pr[0] = pq0;
        pr[1] = pq1;
        a.partials[(size_t)blockIdx.x * kTxFields + 2] = px;
        a.partials[(size_t)blockIdx.x * kTxFields + 3] = mx;
    }
    if constexpr (CLIP) {
        // the record: one 64-bit vector atomic per field and workgroup (integers: any order)
        const unsigned long long nc = block_sum<unsigned long long, BLK>(n_clip, (unsigned long long*)red);
        const unsigned long long ns = block_sum<unsigned long long, BLK>(n_seen, (unsigned long long*)red);
        unsigned long long* rec = tx_tail(tail...).counters;
        if (threadIdx.x == 0 && rec != nullptr) {
            if (nc) atomicAdd(&rec[0], nc);
            if (ns) atomicAdd(&rec[1], ns);
        }
    }
}

// ============================================================ fused RX
// static (__shared__) LDS of k_rx beside its dynamic rows: the noise phase table, and for the
// complex128 throughput kernels the table widened to double (Mwc64x::add_noise64)
template <typename R, int FB>
constexpr int rx_ntab64_static() { return sizeof(R) == 8 && FB > 0 ? kNoisePhases : 1; }
template <typename R, int FB>
constexpr size_t rx_static_lds() { return kNoisePhases * sizeof(f32x2) + rx_ntab64_static<R, FB>() * sizeof(f64x2); }
// per-pass twiddles of a throughput receiver: the forward ones, plus the inverse ones for SC-OFDM's IFFT
template <typename R, int LOGN, int FB>
constexpr int rx_tts(bool scm) {
    constexpr int TTS = uses_tt<R, LOGN, FB>() ? tt_size(LOGN) : 0;
    return FB > 1 && scm ? 2 * TTS : TTS;
}
// The dynamic LDS of k_rx for the plan's staged bit words per symbol and the twiddles the kernel
// stages (rx_tts): the kernel's layout and the launcher's byte count
template <typename R>
struct RxLds {
    // adaptive: per-order slicer constants (complex128: double entries)
    using OP = std::conditional_t<sizeof(R) == 8, OrderParams64, OrderParams>;
    cpx<R> *tw, *tt, *eqt;
    AxisInfo* axis;
    unsigned char* rowmem;
    uint32_t* words;
    R* red;
    unsigned long long* redc;
    OP* ordt;
    uint8_t* wpat;  // wide plan: level -> index bits, [ipat | qpat] of kWideSide bytes per LUT
    // k_rx_sweep: a noise phase table per SNR point (the complex128 throughput form: widened to
    // double, as ntab64) and the workgroup's (bit errors, symbol errors) per point
    f32x2* sntab;
    f64x2* sntab64;
    unsigned long long* scnt;
};
// n_wide (generic kernel): the LUTs of a plan with an order above 256 (side 32 / 64 slicer tables)
// n_sweep (k_rx_sweep): the SNR points of the launch (<= OFDM_MAX_SWEEP_POINTS), 0 in every other kernel
// (ONE_WAVE: the form's workgroup shape, RxFormOf)
template <typename R, int LOGN, int EQ, int FB, bool MV, bool ONE_WAVE, typename CV>
__host__ __device__ __forceinline__ constexpr RxLds<R> rx_carve(CV& cv, int words_per_sym, int tts_all,
                                                                int n_wide = 0, int n_sweep = 0) {
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, ONE_WAVE>();
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr bool SPLIT = split_rows<R, FB>();  // complex128 throughput: rows of reals
    RxLds<R> m{};
    // two-level twiddles (generic kernel, complex128 N > 1024)
    m.tw = cv.template take<C>(uses_tt<R, LOGN, FB>() ? 0 : 128);
    m.axis = cv.template take<AxisInfo>(kMaxLuts);
    m.rowmem = cv.template take<unsigned char>((size_t)G::SPB * G::PADN * (SPLIT ? sizeof(R) : sizeof(C)));
    m.words = cv.template take<uint32_t>(FB ? 0 : (size_t)G::SPB * words_per_sym);  // reference bits
    m.red = cv.template take<R>(BLK / 64);
    m.redc = cv.template take<unsigned long long>(BLK / 64);
    m.tt = cv.template take<C>(tts_all);
    m.ordt = cv.template take<typename RxLds<R>::OP>(FB == 1 ? 8 : 0);
    // throughput kernels with an equaliser: the per-subcarrier coefficient staged in LDS once
    // per workgroup (ZF: 1/H; MMSE: conj(H), |H|^2 recomputed from it) -- read from the plan's
    // global table, every element paid an L2 round trip with a vmcnt(0) per symbol
    m.eqt = cv.template take<C>(eq_in_lds<R, FB, LOGN, EQ>() ? G::N : 0);
    m.wpat = cv.template take<uint8_t>(FB == 0 ? (size_t)n_wide * 2 * kWideSide : 0);
    constexpr bool F64_FAST = sizeof(R) == 8 && FB > 0;
    m.sntab = cv.template take<f32x2>(F64_FAST ? 0 : (size_t)n_sweep * kNoisePhases);
    m.sntab64 = cv.template take<f64x2>(F64_FAST ? (size_t)n_sweep * kNoisePhases : 0);
    m.scnt = cv.template take<unsigned long long>((size_t)n_sweep * 2);
    return m;
}

// EQ: OFDM_EQ_* fixed at compile time (throughput kernel) or -1 = from the plan.
// MV: SC-OFDM and zero padding compiled in (run-time flags); complex128 compiles them out of the
// cyclic-prefix OFDM kernels (rx_eq)
// REF: the throughput kernel fed the caller's bits and normals (reference streams) -- the same body
// WIDE: the generic kernel for a plan with an order above 256 (the side 32 / 64 slicer), an
// instantiation of its own like k_tx's
// PROF: the per-subcarrier profile of the run (RxArgs::profile, ofdm_rx_profile) compiled in.  A lane
// owns the same subcarriers t + i TPS in every symbol it processes, so it keeps their five
// quantities in registers across the symbol loop; at the end the workgroup's symbol slots are summed
// through the FFT rows' LDS and every subcarrier's row gets one 64-bit integer atomic per workgroup.
// Integers only: the record does not depend on the order of arrival, the batching or the rank count.
// The body (ofdm_rx_body.hpp) is shared by k_rx (PROF = false: the code as before) and k_rx_prof.  It
// is included into both kernels, not called: as a __device__ function template, force-inlined, with
// the arguments by reference or by value, it changed the register allocation of 74 existing k_rx
// instantiations (k_rx<float, 12, 2, 8>: 55 -> 107 spilled dwords); included, every one of them
// compiles to the registers, spills and LDS it had.
constexpr int kProfRows = 5;        // bit errors, symbol errors, power limb 0, power limb 1, clipped
constexpr double kProfCap = 0x1p20;  // cap of one sample's |z - c|^2
// throughput receivers with a profile: the plan's LUT pool (unscaled) in static LDS, for the
// transmitted point of an element by its lane byte -- a function-local array, so that only the
// kernels that call it (k_rx_prof, FB > 0) carry it
template <int FB>
constexpr int prof_lut_static() { return FB == 1 ? kMaxLut : (FB > 1 ? (1 << FB) : 0); }
template <typename C, int FB>
__device__ __forceinline__ C* prof_lut() {
    __shared__ C lut_s[prof_lut_static<FB>()];
    return lut_s;
}
// one sample of the profile's error-vector power: e = z - c, capped; a capped or non-finite one is counted
template <typename R>
__device__ __forceinline__ void prof_power(cpx<R> z, cpx<R> c, unsigned long long& l0, unsigned long long& l1,
                                           uint32_t& clipped) {
    const R er = z.re - c.re, ei = z.im - c.im;
    const R p = er * er + ei * ei;
    const bool clip = !(p < (R)kProfCap);
    clipped += clip;
    fx_accum(clip ? (R)kProfCap : p, l0, l1);
}
// The density record's LDS behind rx_carve's layout: G x G 32-bit bins (k_rx_dens and its launcher)
template <typename CV>
__host__ __device__ __forceinline__ constexpr uint32_t* dens_lds(CV& cv, int bins) {
    return cv.template take<uint32_t>((size_t)bins * bins);
}
// One point into the density histogram (ofdm_hip.h, ofdm_rx_density: the index).  Per axis
// t = (c - lo) * inv_w in double, one rounded subtraction and one rounded multiplication (no contraction:
// a NumPy restatement reproduces it bit for bit); inside iff 0 <= t < G on both axes, which a NaN or an
// infinity fails.  Inside: one LDS add without return; otherwise the lane's outside count.
template <typename R>
__device__ __forceinline__ void dens_bin(cpx<R> v, const RxDensTail& dt, uint32_t* hist, unsigned long long& outside) {
#pragma clang fp contract(off)
    const double g = (double)dt.bins;
    const double tr = __dmul_rn(__dsub_rn((double)v.re, dt.lo), dt.inv_w);
    const double ti = __dmul_rn(__dsub_rn((double)v.im, dt.lo), dt.inv_w);
    if (tr >= 0.0 && tr < g && ti >= 0.0 && ti < g)
        __hip_atomic_fetch_add(hist + (int)ti * dt.bins + (int)tr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        ++outside;
}
template <typename R, int LOGN, int EQ, int FB, bool MV, bool REF = false, bool WIDE = false>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Plain>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Plain>::ONE_WAVE>())) void k_rx(
    RxArgs a) {
    using FORM = RxFormOf<RxForm::Plain>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS;
#include "ofdm_rx_body.hpp"
}

// The receiver that also accumulates the per-subcarrier profile: an instantiation of its own, so
// that every k_rx compiles as before.  Instantiated for the generic kernel (and its WIDE form) and
// for the complex128 cyclic-prefix OFDM throughput receivers of the bench shapes (ofdm_record_inst.hpp).
template <typename R, int LOGN, int EQ, int FB, bool MV, bool REF = false, bool WIDE = false>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Prof>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Prof>::ONE_WAVE>())) void k_rx_prof(
    RxArgs a) {
    using FORM = RxFormOf<RxForm::Prof>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS;
#include "ofdm_rx_body.hpp"
}

// The receiver that also accumulates the per-frame error record (ofdm_rx_frames, ofdm_hip.h: the
// definition): k_rx with FRAMES compiled in -- where a symbol's bit and symbol errors are final they are
// summed over the symbol's lanes inside the wave and added to the symbol's frame, at most two 64-bit
// integer atomics per symbol and wave, none for a symbol without errors.  No LDS and no barrier beyond
// k_rx's, so k_rx's own workgroup shapes and waves per SIMD.  The frame arguments are a second kernel
// parameter (RxFramesTail) that only this kernel has: RxArgs and every other receiver stay what they
// were.  Instantiated for the generic kernel (and its WIDE form) and for the complex128 cyclic-prefix
// OFDM throughput receivers of the bench shapes (ofdm_record_inst.hpp).
template <typename R, int LOGN, int EQ, int FB, bool MV, bool WIDE = false>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Frames>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Frames>::ONE_WAVE>())) void k_rx_frames(
    RxArgs a, RxFramesTail ft) {
    using FORM = RxFormOf<RxForm::Frames>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS, REF = false;
#define OFDM_RX_BODY_FRAMES
#include "ofdm_rx_body.hpp"
#undef OFDM_RX_BODY_FRAMES
}

// The receiver that also bins every equalised point into the constellation-density record
// (ofdm_rx_density, ofdm_hip.h: the definition): k_rx with DENS compiled in.  The G x G histogram is
// 32-bit bins in LDS behind the receiver's own layout (dens_lds), zeroed once per workgroup and fed with
// one ds_add_u32 (no return) per binned point; the points outside the square are a per-lane register
// count.  At the end every non-empty bin of the workgroup issues one 64-bit integer atomic into the
// record, and the workgroup's outside count one more.  Integers only: the record does not depend on the
// grid, the batching or the rank count.  The throughput receivers fill the LDS at their own workgroup
// shapes (about 156 of 160 KB at config b's), so the kernel takes the profile's one-wave-per-SIMD shape
// (rx_block / rx_waves with ONE_WAVE), which leaves the histogram its 64 KB.
// The 32-bit bins cannot wrap: one symbol-loop iteration bins at most SPB * N points, and after
// RxDensTail::flush = floor((2^32 - 1) / (SPB * N)) iterations the workgroup adds its bins to the record
// and zeroes them, a barrier on either side (a flush every >= 2^18 iterations: nothing beside a run's
// other work).  The density arguments are a second kernel parameter (RxDensTail) that only this kernel
// has.  Instantiated for the generic kernel (and its WIDE form) and for the complex128 cyclic-prefix OFDM
// throughput receivers of the bench shapes (ofdm_record_inst.hpp).
template <typename R, int LOGN, int EQ, int FB, bool MV, bool WIDE = false>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Dens>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Dens>::ONE_WAVE>())) void k_rx_dens(
    RxArgs a, RxDensTail dt) {
    using FORM = RxFormOf<RxForm::Dens>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS, REF = false;
#define OFDM_RX_BODY_DENS
#include "ofdm_rx_body.hpp"
#undef OFDM_RX_BODY_DENS
}

// The soft-decision record's LDS behind rx_carve's layout (k_rx_soft and its launcher): the plan's level
// table, double[kMaxLuts][2][kSoftSide], then kSoftRows x 2 x B 32-bit bins
struct SoftLds {
    double* lev;
    uint32_t* hist;
};
template <typename CV>
__host__ __device__ __forceinline__ constexpr SoftLds soft_lds(CV& cv, int bins) {
    SoftLds m{};
    m.lev = cv.template take<double>((size_t)kMaxLuts * 2 * kSoftSide);
    m.hist = cv.template take<uint32_t>((size_t)kSoftRows * 2 * bins);
    return m;
}
// One element into the soft-decision histogram (ofdm_hip_soft.h, ofdm_rx_soft: the definition).  Per axis the
// squared distances to the side levels, each fl(fl(c - lev) * fl(c - lev)) in double with no contraction,
// and per bit of the axis the minimum over the levels whose index has the bit clear and set; then
// D = fl(m1 - m0), u = fl(D * g), t = fl(u * inv_w), binned at B/2 + floor(t), clamped in double.  A
// straight scan over the levels: the minima are exact selections, so their order does not matter, and a
// NumPy restatement reproduces every double bit for bit.
//   HBMAX: the most bits per axis the instantiation can meet (the loops' compile-time bound)
//   lev: the LUT's [2][kSoftSide] levels in LDS; tidx: the transmitted index; cmask: its compared bits
template <int HBMAX, typename R>
__device__ __forceinline__ void soft_bin(cpx<R> v, int hb, uint32_t tidx, uint32_t cmask, const double* lev, double gk,
                                         const RxSoftTail& st, uint32_t* hist, unsigned long long& invalid) {
#pragma clang fp contract(off)
    const int side = 1 << hb, half = st.bins >> 1;
    const int row0 = hb * (hb - 1) + 2 * hb - 1;  // the row of index bit 0 (the last bit, MSB first)
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        // ax = 0: the Q axis, index bits hb .. 2 hb - 1; ax = 1: the I axis, index bits 0 .. hb - 1
        const double c = ax == 0 ? (double)v.im : (double)v.re;
        const double* const l = lev + (ax == 0 ? kSoftSide : 0);
        double m0[HBMAX], m1[HBMAX];
#pragma unroll
        for (int p = 0; p < HBMAX; ++p) m0[p] = m1[p] = (double)INFINITY;
#pragma unroll
        for (int a = 0; a < (1 << HBMAX); ++a) {
            if (a < side) {
                const double e = __dsub_rn(c, l[a]);
                const double d = __dmul_rn(e, e);
#pragma unroll
                for (int p = 0; p < HBMAX; ++p) {
                    if ((a >> p) & 1)
                        m1[p] = __builtin_fmin(m1[p], d);
                    else
                        m0[p] = __builtin_fmin(m0[p], d);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < HBMAX; ++p) {
            const int pos = (ax == 0 ? hb : 0) + p;  // the bit's position in the index
            if (p < hb && ((cmask >> pos) & 1u)) {
                const double t = __dmul_rn(__dmul_rn(__dsub_rn(m1[p], m0[p]), gk), st.inv_w);
                if (t != t) {
                    ++invalid;
                } else {
                    double f = __builtin_floor(t);
                    f = f < (double)-half ? (double)-half : f;
                    f = f > (double)(half - 1) ? (double)(half - 1) : f;
                    const int bin = half + (int)f;
                    const int cell = ((row0 - pos) * 2 + (int)((tidx >> pos) & 1u)) * st.bins + bin;
                    __hip_atomic_fetch_add(hist + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
}

// soft_bin out of line, for the generic kernel: inlined into its element loop the scan changes how the
// compiler unswitches and schedules the loop, and with that which products of the complex64 equaliser
// become FMAs -- the tap of k_rx_soft would differ from k_rx's in the last bit.  Behind a call the loop
// keeps k_rx's arithmetic.
template <typename R>
__device__ __noinline__ void soft_bin_call(cpx<R> v, int hb, uint32_t tidx, uint32_t cmask, const double* lev, double gk,
                                           const RxSoftTail& st, uint32_t* hist, unsigned long long& invalid) {
    soft_bin<4, R>(v, hb, tidx, cmask, lev, gk, st, hist, invalid);
}

// The receiver that also accumulates the soft-decision record (ofdm_rx_soft, ofdm_hip_soft.h: the definition):
// k_rx with the soft section compiled in.  Where the density bins the point, this form takes the same
// point, the element's transmitted index (the one the symbol-error count compares) and its compared-bit
// mask, and adds one count per compared bit to a [20][2][B] histogram of 32-bit bins in LDS behind the
// receiver's own layout (soft_lds: the plan's level table staged in front of it).  Flushed and ended as
// k_rx_dens' histogram is: one 64-bit integer atomic per non-empty bin and workgroup, a flush before a bin
// could wrap (one iteration adds at most SPB * N to a bin), the NaN count a per-lane register.  Integers
// only.  It takes the density's one-wave-per-SIMD shape, instantiations and routing; a WIDE plan has no
// form (refused by the ABI).
template <typename R, int LOGN, int EQ, int FB, bool MV, bool WIDE = false>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Soft>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Soft>::ONE_WAVE>())) void k_rx_soft(
    RxArgs a, RxSoftTail st) {
    using FORM = RxFormOf<RxForm::Soft>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS, REF = false;
#define OFDM_RX_BODY_SOFT
#include "ofdm_rx_body.hpp"
#undef OFDM_RX_BODY_SOFT
}

// The one-pass SNR sweep receiver (ofdm_rx_sweep): every symbol is received once per SNR point of the
// launch -- y read, the lane block and the noise words drawn once per symbol; per point the noise
// scaled by the point's phase table, then the FFT, MMSE variance, equaliser, slicer and count of k_rx
// (the same body), so that point k's counts are those of a k_rx launch at snr_db[k].  Throughput
// streams only.  Instantiated for the generic kernel (FB = 0: every plan that runs Philox streams) and
// for the complex128 cyclic-prefix OFDM fixed-QAM bench shapes (ofdm_sweep_inst.hpp); the throughput
// form keeps y (64 VGPRs), the radii and the phase words in registers across the points, so it takes
// the profile's one-wave-per-SIMD workgroup shape (rx_block / rx_waves with ONE_WAVE).
template <typename R, int LOGN, int EQ, int FB, bool MV>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Sweep>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::Sweep>::ONE_WAVE>())) void k_rx_sweep(
    RxSweepArgs sa) {
    using FORM = RxFormOf<RxForm::Sweep>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS, REF = false, WIDE = false;
    const RxArgs& a = sa.r;  // (a copy of its own that took each point's snr_lin in turn left the argument registers for memory)
#define OFDM_RX_BODY_SWEEP
#include "ofdm_rx_body.hpp"
#undef OFDM_RX_BODY_SWEEP
}

// The sweep receiver that also accumulates the per-frame error record of every point
// (ofdm_rx_sweep_frames, ofdm_hip_sweep_frames.h: the definition): k_rx_sweep with k_rx_frames' frame block compiled
// into the point loop.  There bes / ses are the symbol's counts at the point, so the block is what it
// is in k_rx_frames -- the segment sum over the symbol's lanes, then one 64-bit integer atomic per
// non-zero field from the segment's first lane -- into row pt * n_frames + frame of a point-major record.
// counters[n_snr][2] stay the sweep's per-point pairs in lds.scnt: where a symbol is whole waves (N >= 1024)
// the frame block's wave sum feeds them and the sweep's own 64-lane __shfl_xor sum is compiled out; where
// several symbols share a wave the segment sums are not mixed and the sweep's own sum stays.
// No LDS and no barrier beyond k_rx_sweep's, so its workgroup shapes, waves per SIMD and grid.  The frame
// arguments are the trailing kernel parameter (RxFramesTail, as k_rx_frames'): RxSweepArgs and every
// other receiver stay what they were.  Instantiated as k_rx_sweep is (ofdm_sweep_inst.hpp: one routing).
template <typename R, int LOGN, int EQ, int FB, bool MV>
__global__ __launch_bounds__((rx_block<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::SweepFrames>::ONE_WAVE>()),
                             (rx_waves<R, FB, LOGN, EQ, MV, RxFormOf<RxForm::SweepFrames>::ONE_WAVE>())) void k_rx_sweep_frames(
    RxSweepArgs sa, RxFramesTail ft) {
    using FORM = RxFormOf<RxForm::SweepFrames>;
    constexpr bool PROF = FORM::PROF, SWEEP = FORM::SWEEP, FRAMES = FORM::FRAMES, DENS = FORM::DENS, REF = false, WIDE = false;
    const RxArgs& a = sa.r;  // (as k_rx_sweep)
#define OFDM_RX_BODY_SWEEP
#define OFDM_RX_BODY_FRAMES
#include "ofdm_rx_body.hpp"
#undef OFDM_RX_BODY_FRAMES
#undef OFDM_RX_BODY_SWEEP
}

}  // namespace ofdm
