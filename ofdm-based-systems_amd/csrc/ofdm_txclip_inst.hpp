// ofdm_txclip_inst.hpp -- the clipped transmitter (ofdm_tx_clip): the CLIP instantiations of k_tx, their
// launcher and the routing predicates beside it; included once per precision by
// ofdm_kernels_f32_txclip.hip / ofdm_kernels_f64_txclip.hip, translation units of their own beside the
// k_tx / k_rx / k_rx_prof / k_rx_sweep / k_link / k_papr ones (every other object stays as it was).
//
// The kernel is k_tx with the limiter compiled in (ofdm_fused.hpp, CLIP; its arguments a second kernel
// parameter, TxClipTail): the same map, IFFT, prefix, FIR, tails and statistics on the same templates,
// the same workgroup shapes, LDS layout (tx_carve: the record's reduction reuses the partials' scratch,
// no new LDS) and grid.
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// tx_launch with the limiter's arguments (FB > 0: a throughput form; its LDS not fitting, the generic form)
template <typename R, int LOGN, int FB, int LT>
static hipError_t tx_clip_launch(const TxArgs& a0, const TxClipTail& k0, double a2_h0, int* grid, hipStream_t s) {
    constexpr int BLK = tx_block<R, FB, LOGN, LT>();
    TxArgs a = a0;
    TxClipTail k = k0;
    a.slot = tx_row_slot<R, LOGN, FB, LT>(a.slot, a.c.cp);
    CarveSize lds;
    tx_carve<R, LOGN, FB, LT, BLK>(lds, a.c.lut_len, a.c.words_per_sym, tx_tails(a.L), a.slot, 0);
    const size_t sm = lds.bytes;
    if (sm + tx_static_lds<R, FB, LT>() > kLdsPerCu) {
        if constexpr (FB > 0) return tx_clip_launch<R, LOGN, 0, -1>(a0, k0, a2_h0, grid, s);
        else return kLdsOverflow;
    }
    // the flat throughput form's symbol leaves the IFFT as h0 x: |h0 x|^2 against A2 |h0|^2 (one tap,
    // so |h0|^2 = 1 up to rounding; no other form reads a2_h0 -- a channel whose first tap is 0 has L > 1)
    if constexpr (FB > 0 && LT == 0) {
        if (!(a2_h0 > 0.0)) return hipErrorInvalidValue;
        k.a2 = a2_h0;
    }
    return tx_go<BLK, Geo<LOGN, BLK>::SPB>(k_tx<R, LOGN, FB, LT, false, false, false, true, TxClipTail>, sm, a, grid, s,
                                           k);
}

// Routing, the one definition: the throughput forms take the two complex128 N = 1024 64-QAM bench shapes
// (bench_fixed_shape<6>: cyclic-prefix OFDM or no prefix) on Philox streams -- a flat channel (configs b:
// k_tx<double, 10, 6, 0>) and 2 to 8 taps within the window FIR's reach, cp <= TPS (config c:
// k_tx<double, 10, 6, 8>, the taps zero past L) -- and the generic form every other plan: any caller
// bits (no REF x CLIP kernels), complex64, SC-OFDM, zero padding, adaptive loading, PSK, configs d / e.
template <typename R, int LOGN>
constexpr bool clip_fast_n() { return sizeof(R) == 8 && LOGN == 10 && ref_fb<R, LOGN>() == 6; }
template <typename R, int LOGN>
static bool clip_fast_shape(const TxArgs& a) {
    if constexpr (!clip_fast_n<R, LOGN>()) return false;
    else return a.c.bits == nullptr && bench_fixed_shape<6>(a.c);
}
static inline bool clip_flat(const TxArgs& a) { return a.L == 1; }
template <int LOGN>
static bool clip_window(const TxArgs& a) { return a.L > 1 && a.L <= 8 && a.c.cp <= Geo<LOGN>::TPS; }

template <typename R, int LOGN>
static hipError_t tx_clip_one(const TxArgs& a, const TxClipTail& k, double a2_h0, int* grid, hipStream_t s) {
    if constexpr (clip_fast_n<R, LOGN>()) {
        if (clip_fast_shape<R, LOGN>(a)) {
            if (clip_flat(a)) return tx_clip_launch<R, LOGN, 6, 0>(a, k, a2_h0, grid, s);
            if (clip_window<LOGN>(a)) return tx_clip_launch<R, LOGN, 6, 8>(a, k, a2_h0, grid, s);
        }
    }
    return tx_clip_launch<R, LOGN, 0, -1>(a, k, a2_h0, grid, s);
}

template <typename R>
hipError_t launch_tx_clip(int logn, const TxArgs& a, double a2, double a2_h0, unsigned long long* counters, int* grid,
                          hipStream_t s) {
    if (a.wide != nullptr || !(a2 > 0.0)) return hipErrorInvalidValue;
    TxClipTail k{};
    k.a2 = a2;
    k.counters = counters;
    return with_logn(logn, [&](auto l) { return tx_clip_one<R, decltype(l)::value>(a, k, a2_h0, grid, s); });
}

#define OFDM_INSTANTIATE_TXCLIP(R) \
    template hipError_t launch_tx_clip<R>(int, const TxArgs&, double, double, unsigned long long*, int*, hipStream_t);

}  // namespace ofdm
