// complex64 instantiation of the clipped transmitter's launcher (k_tx CLIP).
#include "ofdm_txclip_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_TXCLIP(float)
}  // namespace ofdm
