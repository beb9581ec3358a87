// complex128 instantiation of the SNR sweep RX launcher with the frame record (every k_rx_sweep_frames
// specialisation).
#include "ofdm_sweepframes_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_SWEEP_FRAMES(double)
}  // namespace ofdm
