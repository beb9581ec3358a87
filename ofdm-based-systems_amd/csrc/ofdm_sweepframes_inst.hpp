// ofdm_sweepframes_inst.hpp -- launcher of the one-pass SNR sweep receiver with the per-frame error record
// of every point (ofdm_rx_sweep_frames); included once per precision by ofdm_kernels_f32_sweepframes.hip /
// ofdm_kernels_f64_sweepframes.hip, translation units of their own beside the k_rx_sweep / k_rx_frames
// ones (every other object stays as it was).
#pragma once

#include "ofdm_sweep_inst.hpp"

namespace ofdm {

// Routing, LDS layout, workgroup shape and grid are launch_rx_sweep's (rx_sweep_one with the frame tail:
// the six complex128 fixed-QAM throughput forms, everything else the generic one); the record needs no
// LDS.  The frame arguments were checked once, by the ABI (ofdm_abi.hip frames_ok).
template <typename R>
hipError_t launch_rx_sweep_frames(int logn, const RxSweepArgs& a, const RxFramesTail& f, hipStream_t s) {
    if (!rx_sweep_args_ok(a)) return hipErrorInvalidValue;
    return with_logn(logn, [&](auto l) { return rx_sweep_one<R, decltype(l)::value>(a, s, f); });
}

#define OFDM_INSTANTIATE_RX_SWEEP_FRAMES(R) \
    template hipError_t launch_rx_sweep_frames<R>(int, const RxSweepArgs&, const RxFramesTail&, hipStream_t);

}  // namespace ofdm
