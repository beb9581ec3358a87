// complex128 instantiation of the SNR sweep RX launcher (every k_rx_sweep specialisation).
#include "ofdm_sweep_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_SWEEP(double)
}  // namespace ofdm
