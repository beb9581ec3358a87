// complex64 instantiation of the per-symbol PAPR histogram launcher (k_papr).
#include "ofdm_papr_inst.hpp"

namespace ofdm {
OFDM_INSTANTIATE_PAPR(float)
}  // namespace ofdm
