// complex128 instantiation of the profiling RX launcher (every k_rx_prof specialisation).
#include "ofdm_record_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_RX_PROF(double)
}  // namespace ofdm
