// ofdm_prof_inst.hpp -- launcher of the receiver with the per-subcarrier profile (ofdm_rx_profile);
// included once per precision by ofdm_kernels_f32_prof.hip / ofdm_kernels_f64_prof.hip, translation
// units of their own beside the k_rx ones (parallel compile, and every k_rx object stays as it was).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// Routing with a profile (the predicates: ofdm_kernels_inst.hpp): a bench shape with Philox streams takes
// its throughput receiver's k_rx_prof, by equaliser.  Everything else takes the generic kernel's
// (EQ = -1, FB = 0): caller bits, caller normals or a tap (the bench shapes included), complex64, every
// other shape; a plan with an order above 256 its WIDE form.  The REF instantiations have no profile.
template <typename R, int LOGN, int EQ, int FB, bool WIDE = false>
static hipError_t rx_prof_launch(const RxArgs& a, hipStream_t s) {
    constexpr bool MV = FB <= 1;  // (as rx_one: compiled out of the fixed-QAM kernels; FB = 1 switches it off)
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, true>();
    CarveSize lds;
    // (the profile's symbol slots reuse the FFT rows: no dynamic LDS beyond the receiver's own)
    rx_carve<R, LOGN, EQ, FB, MV, true>(lds, a.c.words_per_sym, rx_tts<R, LOGN, FB>(a.c.scm), WIDE ? a.c.n_axis : 0);
    if (lds.bytes + rx_static_lds<R, FB>() + prof_lut_static<FB>() * sizeof(cpx<R>) > kLdsPerCu) {
        // (a layout that does not fit: the generic kernel, as the throughput receivers without a profile)
        if constexpr (FB > 0) return rx_prof_launch<R, LOGN, -1, 0>(a, s);
        else return kLdsOverflow;
    }
    // Every workgroup ends with up to five atomics per subcarrier: two rounds of the resident workgroups
    return rx_go<BLK, Geo<LOGN, BLK>::SPB>(k_rx_prof<R, LOGN, EQ, FB, MV, false, WIDE>, lds.bytes, 2, a.c.n_sym, a, s);
}

template <typename R, int LOGN>
static hipError_t rx_prof_one(const RxArgs& a, hipStream_t s) {
    if constexpr (ref_fb<R, LOGN>() > 0) {
        if (philox_streams(a) && a.wide == nullptr && bench_shape<R, LOGN>(a.c))
            return with_eq(a.c.eq, [&](auto eq) {
                return rx_prof_launch<R, LOGN, decltype(eq)::value, ref_fb<R, LOGN>()>(a, s);
            });
    }
    if (a.wide != nullptr) return rx_prof_launch<R, LOGN, -1, 0, true>(a, s);
    return rx_prof_launch<R, LOGN, -1, 0>(a, s);
}

template <typename R>
hipError_t launch_rx_prof(int logn, const RxArgs& a, hipStream_t s) {
    if (a.profile == nullptr) return hipErrorInvalidValue;
    return with_logn(logn, [&](auto l) { return rx_prof_one<R, decltype(l)::value>(a, s); });
}

#define OFDM_INSTANTIATE_RX_PROF(R) template hipError_t launch_rx_prof<R>(int, const RxArgs&, hipStream_t);

}  // namespace ofdm
