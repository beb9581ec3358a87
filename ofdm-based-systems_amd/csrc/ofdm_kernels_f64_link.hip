// complex128 instantiation of the fused link launcher (k_link: transmit and receive in one kernel).
#include "ofdm_link_inst.hpp"

namespace ofdm {
template hipError_t launch_link<double>(int, int, const LinkArgs&, int, hipStream_t);
}  // namespace ofdm
