// ofdm_frames_inst.hpp -- launcher of the receiver with the per-frame error record (ofdm_rx_frames);
// included once per precision by ofdm_kernels_f32_frames.hip / ofdm_kernels_f64_frames.hip, translation
// units of their own beside the k_tx / k_rx / k_rx_prof / k_rx_sweep / k_link / k_papr ones (every other
// object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing with a frame record (the predicates: ofdm_kernels_inst.hpp): a bench shape with Philox streams
// takes its throughput receiver's k_rx_frames, by equaliser, in k_rx's own workgroup shape, waves per
// SIMD and grid (the record adds no per-element state, unlike the profile).  Everything else takes the
// generic kernel's (EQ = -1, FB = 0): caller bits, caller normals or a tap (the bench shapes included),
// complex64, every other shape; a plan with an order above 256 its WIDE form.  The REF instantiations
// have no frame record.
template <typename R, int LOGN, int EQ, int FB, bool WIDE = false>
static hipError_t rx_frames_launch(const RxArgs& a, const RxFramesTail& f, hipStream_t s) {
    constexpr bool MV = FB <= 1;  // (as rx_one: compiled out of the fixed-QAM kernels; FB = 1 switches it off)
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV>();
    CarveSize lds;
    rx_carve<R, LOGN, EQ, FB, MV>(lds, a.c.words_per_sym, rx_tts<R, LOGN, FB>(a.c.scm), WIDE ? a.c.n_axis : 0);
    if (lds.bytes + rx_static_lds<R, FB>() > kLdsPerCu) {
        // (a layout that does not fit: the generic kernel, as the throughput receivers without a record)
        if constexpr (FB > 0) return rx_frames_launch<R, LOGN, -1, 0>(a, f, s);
        else return kLdsOverflow;
    }
    return rx_go<BLK, Geo<LOGN, BLK>::SPB>(k_rx_frames<R, LOGN, EQ, FB, MV, WIDE>, lds.bytes,
                                           rx_grid_rounds<R, FB, LOGN>(), a.c.n_sym, a, s, f);
}

template <typename R, int LOGN>
static hipError_t rx_frames_one(const RxArgs& a, const RxFramesTail& f, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        if (philox_streams(a) && a.wide == nullptr && bench_shape<R, LOGN>(a.c))
            return with_eq(a.c.eq, [&](auto eq) {
                return rx_frames_launch<R, LOGN, decltype(eq)::value, ref_fb<R, LOGN>()>(a, f, s);
            });
    }
    if (a.wide != nullptr) return rx_frames_launch<R, LOGN, -1, 0, true>(a, f, s);
    return rx_frames_launch<R, LOGN, -1, 0>(a, f, s);
}

template <typename R>
hipError_t launch_rx_frames(int logn, const RxArgs& a, const RxFramesTail& f, hipStream_t s) {
    // (the frame arguments were checked once, by the ABI: ofdm_abi.hip frames_ok)
    return with_logn(logn, [&](auto l) { return rx_frames_one<R, decltype(l)::value>(a, f, s); });
}

#define OFDM_INSTANTIATE_RX_FRAMES(R) \
    template hipError_t launch_rx_frames<R>(int, const RxArgs&, const RxFramesTail&, hipStream_t);

}  // namespace ofdm
