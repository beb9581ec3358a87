// complex128 instantiation of the soft-decision RX launcher (every k_rx_soft specialisation).
#include "ofdm_record_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_SOFT(double)
}  // namespace ofdm
