// ofdm_sweep_inst.hpp -- launcher of the one-pass SNR sweep receiver (ofdm_rx_sweep); included once
// per precision by ofdm_kernels_f32_sweep.hip / ofdm_kernels_f64_sweep.hip, translation units of their
// own beside the k_rx and k_rx_prof ones (parallel compile, and every other object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing (the predicates: ofdm_kernels_inst.hpp): the fixed-QAM bench shapes (ref_fb > 1) take their
// throughput receiver's k_rx_sweep, by equaliser.  Everything else takes the generic kernel's (EQ = -1,
// FB = 0): complex64, SC-OFDM, zero padding, PSK, N < 64, adaptive plans (one plan for every point:
// adaptive loading re-derived per SNR is a different plan per point and not a sweep).
// tail: nothing (k_rx_sweep), or the frame record's RxFramesTail (k_rx_sweep_frames,
// ofdm_sweepframes_inst.hpp) -- one routing, one layout and one grid for both.
// (the size, fall back, go: rx_form_launch)
template <typename R, int LOGN, int EQ, int FB, typename... T>
static hipError_t rx_sweep_launch(const RxSweepArgs& a, hipStream_t s, const T&... tail) {
    constexpr bool MV = FB == 0;  // (the generic kernel as rx_one launches it; compiled out of the fixed-QAM ones)
    constexpr RxForm F = sizeof...(T) == 0 ? RxForm::Sweep : RxForm::SweepFrames;
    return rx_form_launch<F, R, LOGN, EQ, FB, MV>(a, s, tail...);
}

template <typename R, int LOGN, typename... T>
static hipError_t rx_sweep_one(const RxSweepArgs& a, hipStream_t s, const T&... tail) {
    if constexpr (ref_fb<R, LOGN>() > 1) {
        // (zero_tie: an MMSE plan with a null bin decides its exact zeros in the generic kernel, RxArgs)
        if (bench_fixed_shape<ref_fb<R, LOGN>()>(a.r.c) && !a.r.zero_tie)
            return with_eq(a.r.c.eq, [&](auto eq) {
                return rx_sweep_launch<R, LOGN, decltype(eq)::value, ref_fb<R, LOGN>()>(a, s, tail...);
            });
    }
    return rx_sweep_launch<R, LOGN, -1, 0>(a, s, tail...);
}

// the points and the plan a sweep launch takes (launch_rx_sweep, launch_rx_sweep_frames)
static inline bool rx_sweep_args_ok(const RxSweepArgs& a) {
    return a.n_snr >= 1 && a.n_snr <= OFDM_MAX_SWEEP_POINTS && a.r.wide == nullptr;
}

template <typename R>
hipError_t launch_rx_sweep(int logn, const RxSweepArgs& a, hipStream_t s) {
    if (!rx_sweep_args_ok(a)) return hipErrorInvalidValue;
    return with_logn(logn, [&](auto l) { return rx_sweep_one<R, decltype(l)::value>(a, s); });
}

#define OFDM_INSTANTIATE_RX_SWEEP(R) \
    template hipError_t launch_rx_sweep<R>(int, const RxSweepArgs&, hipStream_t);

}  // namespace ofdm
