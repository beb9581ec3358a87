// ofdm_record_inst.hpp -- launchers of the receivers with a record: the per-subcarrier profile
// (ofdm_rx_profile), the per-frame errors (ofdm_rx_frames), the constellation density (ofdm_rx_density) and
// the soft decisions (ofdm_rx_soft);
// included once per precision and record by ofdm_kernels_f{32,64}_{prof,frames,dens,soft}.hip, translation
// units of their own beside the k_tx / k_rx / k_rx_sweep / k_link / k_papr ones (parallel compile; each
// instantiates its own record's launcher only).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing with a record, one for the four (the predicates: ofdm_kernels_inst.hpp): a bench shape with
// Philox streams takes its throughput receiver's k_rx_prof / k_rx_frames / k_rx_dens / k_rx_soft, by equaliser.
// Everything else takes the generic kernel's (EQ = -1, FB = 0): caller bits, caller normals or a tap (the
// bench shapes included), complex64, every other shape; a plan with an order above 256 its WIDE form.  The
// REF instantiations have no record.
//   - the profile, the density and the soft record run in the one-wave-per-SIMD workgroup shape, the frame record in k_rx's
//     own workgroup shape, waves per SIMD and grid: it adds no per-element state (RxFormOf, rx_form_launch);
//   - a density or soft call with z_out takes the generic kernel even when z_keep is 0 (philox_streams), so
//     that a run with a tap holds one form over all its batches;
//   - the soft record has no WIDE form: the ABI refuses a plan with an order above 256 before the launcher.
template <RxForm F, typename R, int LOGN, int EQ, int FB, bool WIDE = false, typename... T>
static hipError_t rx_record_launch(const RxArgs& a, hipStream_t s, const T&... tail) {
    constexpr bool MV = FB <= 1;  // (as rx_one: compiled out of the fixed-QAM kernels; FB = 1 switches it off)
    return rx_form_launch<F, R, LOGN, EQ, FB, MV, false, WIDE>(a, s, tail...);
}

template <RxForm F, typename R, int LOGN, typename... T>
static hipError_t rx_record_one(const RxArgs& a, hipStream_t s, const T&... tail) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        if (philox_streams(a) && a.wide == nullptr && bench_shape<R, LOGN>(a.c))
            return with_eq(a.c.eq, [&](auto eq) {
                return rx_record_launch<F, R, LOGN, decltype(eq)::value, ref_fb<R, LOGN>()>(a, s, tail...);
            });
    }
    if constexpr (F == RxForm::Soft) {
        if (a.wide != nullptr) return hipErrorInvalidValue;
    } else {
        if (a.wide != nullptr) return rx_record_launch<F, R, LOGN, -1, 0, true>(a, s, tail...);
    }
    return rx_record_launch<F, R, LOGN, -1, 0>(a, s, tail...);
}

template <typename R>
hipError_t launch_rx_prof(int logn, const RxArgs& a, hipStream_t s) {
    if (a.profile == nullptr) return hipErrorInvalidValue;
    return with_logn(logn, [&](auto l) { return rx_record_one<RxForm::Prof, R, decltype(l)::value>(a, s); });
}

template <typename R>
hipError_t launch_rx_frames(int logn, const RxArgs& a, const RxFramesTail& f, hipStream_t s) {
    // (the frame arguments were checked once, by the ABI: ofdm_abi.hip frames_ok)
    return with_logn(logn, [&](auto l) { return rx_record_one<RxForm::Frames, R, decltype(l)::value>(a, s, f); });
}

template <typename R>
hipError_t launch_rx_dens(int logn, const RxArgs& a, const RxDensTail& d, hipStream_t s) {
    // (the density arguments were checked once, by the ABI: ofdm_abi.hip dens_ok; flush: rx_form_launch's)
    return with_logn(logn, [&](auto l) { return rx_record_one<RxForm::Dens, R, decltype(l)::value>(a, s, d); });
}

template <typename R>
hipError_t launch_rx_soft(int logn, const RxArgs& a, const RxSoftTail& t, hipStream_t s) {
    // (the soft arguments and the plan's orders were checked once, by the ABI: ofdm_abi.hip soft_ok; flush:
    // rx_form_launch's)
    return with_logn(logn, [&](auto l) { return rx_record_one<RxForm::Soft, R, decltype(l)::value>(a, s, t); });
}

#define OFDM_INSTANTIATE_RX_PROF(R) template hipError_t launch_rx_prof<R>(int, const RxArgs&, hipStream_t);
#define OFDM_INSTANTIATE_RX_FRAMES(R) \
    template hipError_t launch_rx_frames<R>(int, const RxArgs&, const RxFramesTail&, hipStream_t);
#define OFDM_INSTANTIATE_RX_DENS(R) \
    template hipError_t launch_rx_dens<R>(int, const RxArgs&, const RxDensTail&, hipStream_t);
#define OFDM_INSTANTIATE_RX_SOFT(R) \
    template hipError_t launch_rx_soft<R>(int, const RxArgs&, const RxSoftTail&, hipStream_t);

}  // namespace ofdm
