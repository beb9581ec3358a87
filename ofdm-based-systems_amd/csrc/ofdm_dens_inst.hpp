// ofdm_dens_inst.hpp -- launcher of the receiver with the constellation-density record
// (ofdm_rx_density); included once per precision by ofdm_kernels_f32_dens.hip / ofdm_kernels_f64_dens.hip,
// translation units of their own beside the k_tx / k_rx / k_rx_prof / k_rx_frames / k_rx_sweep / k_link /
// k_papr ones (every other object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing with a density record is the profile's (rx_prof_one; the predicates: ofdm_kernels_inst.hpp): a
// bench shape with Philox streams takes its throughput receiver's k_rx_dens, by equaliser, in the
// profile's one-wave-per-SIMD workgroup shape.  Everything else takes the generic kernel's (EQ = -1,
// FB = 0): caller bits, caller normals, a call with z_out (philox_streams: even when z_keep is 0, so that a
// run with a tap holds one form over all its batches), complex64, every other shape; a plan with an order
// above 256 its WIDE form.  The REF instantiations have no density record.
template <typename R, int LOGN, int EQ, int FB, bool WIDE = false>
static hipError_t rx_dens_launch(const RxArgs& a, RxDensTail d, hipStream_t s) {
    constexpr bool MV = FB <= 1;  // (as rx_one: compiled out of the fixed-QAM kernels; FB = 1 switches it off)
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, true>();
    using G = Geo<LOGN, BLK>;
    CarveSize lds;
    rx_carve<R, LOGN, EQ, FB, MV, true>(lds, a.c.words_per_sym, rx_tts<R, LOGN, FB>(a.c.scm), WIDE ? a.c.n_axis : 0);
    dens_lds(lds, d.bins);  // the histogram behind the receiver's own layout, as the kernel carves it
    if (lds.bytes + rx_static_lds<R, FB>() > kLdsPerCu) {
        // (a layout that does not fit: the generic kernel, as the throughput receivers without a record)
        if constexpr (FB > 0) return rx_dens_launch<R, LOGN, -1, 0>(a, d, s);
        else return kLdsOverflow;
    }
    // one iteration of a workgroup bins at most SPB * N points (<= 16384): the 32-bit bins are flushed
    // every `flush` iterations, before any of them could reach 2^32 (k_rx_dens)
    d.flush = (uint32_t)(0xFFFFFFFFull / ((unsigned long long)G::SPB * G::N));
    // Every workgroup ends with up to one atomic per bin: two rounds of the resident workgroups, as the profile
    return rx_go<BLK, G::SPB>(k_rx_dens<R, LOGN, EQ, FB, MV, WIDE>, lds.bytes, 2, a.c.n_sym, a, s, d);
}

template <typename R, int LOGN>
static hipError_t rx_dens_one(const RxArgs& a, const RxDensTail& d, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        if (philox_streams(a) && a.wide == nullptr && bench_shape<R, LOGN>(a.c))
            return with_eq(a.c.eq, [&](auto eq) {
                return rx_dens_launch<R, LOGN, decltype(eq)::value, ref_fb<R, LOGN>()>(a, d, s);
            });
    }
    if (a.wide != nullptr) return rx_dens_launch<R, LOGN, -1, 0, true>(a, d, s);
    return rx_dens_launch<R, LOGN, -1, 0>(a, d, s);
}

template <typename R>
hipError_t launch_rx_dens(int logn, const RxArgs& a, const RxDensTail& d, hipStream_t s) {
    // (the density arguments were checked once, by the ABI: ofdm_abi.hip dens_ok)
    return with_logn(logn, [&](auto l) { return rx_dens_one<R, decltype(l)::value>(a, d, s); });
}

#define OFDM_INSTANTIATE_RX_DENS(R) \
    template hipError_t launch_rx_dens<R>(int, const RxArgs&, const RxDensTail&, hipStream_t);

}  // namespace ofdm
