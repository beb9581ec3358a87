// complex128 instantiation of the frame-record RX launcher (every k_rx_frames specialisation).
#include "ofdm_record_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_FRAMES(double)
}  // namespace ofdm
