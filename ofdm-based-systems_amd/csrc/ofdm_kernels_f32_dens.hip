// complex64 instantiation of the density-record RX launcher (every k_rx_dens specialisation).
#include "ofdm_record_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_DENS(float)
}  // namespace ofdm
