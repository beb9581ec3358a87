/*
 * ofdm_hip_soft.h -- an extension header of libofdm_hip's C ABI (include/ofdm_hip.h, ABI 6): the receiver
 * with the soft-decision record.  The entry point lives in the same library; ofdm_hip.h, its types, its
 * constants and every entry point it declares are as they were.
 */
#ifndef OFDM_HIP_SOFT_H
#define OFDM_HIP_SOFT_H

#include "ofdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bins of ofdm_rx_soft's histograms at most (even, at least 2): the kernel's histogram is 40 * B 32-bit
 * bins in LDS, 40 KB at 256. */
#define OFDM_MAX_SOFT_BINS 256
/* Rows of ofdm_rx_soft's record: one per bit of the four square-QAM orders, 2 + 4 + 6 + 8 */
#define OFDM_SOFT_ROWS 20

/*
 * ofdm_rx with a soft-decision record of the run (an entry point added to ABI 6: nothing of the version's
 * existing interface changes, so the number stands): for every compared bit of every active subcarrier
 * the max-log distance difference, binned into a histogram conditioned on the transmitted bit.
 *
 * Scope: plans whose LUTs are all separable square QAM of order 4, 16, 64 or 256 (fixed or adaptive with
 * mixed orders); any prefix, OFDM or SC-OFDM, both precisions.
 * The point: for an element on subcarrier k with b = b_k bits (hb = b / 2, side = 2^hb), v is the point
 * ofdm_rx_density bins for that element -- the value the tap stores in the generic form, the point
 * ofdm_rx_profile forms in the throughput forms -- widened to double (exact).
 * The bits: bit i of the b-bit index, MSB first, i = 0 .. b - 1.  Bits i < hb belong to the Q axis: index
 * a = idx >> hb, level LUT[a << hb].im, component c = v.im, j = i.  Bits i >= hb belong to the I axis:
 * a = idx & (side - 1), level LUT[a].re, c = v.re, j = i - hb.  The levels are the doubles of the LUT the
 * plan was created with (a plan-scoped table of 16 doubles per LUT and axis), not recomputed.
 * The operations, each one separately rounded IEEE double operation, never contracted into an FMA:
 *   d_a = fl(fl(c - lev_a) * fl(c - lev_a))            for each a in [0, side)
 *   m_0 = min over the a whose bit j (MSB first within hb) is 0, m_1 likewise for 1
 *   D = fl(m_1 - m_0)                                  (D > 0: bit 0 is the likelier)
 *   u = fl(D * g[k]),  t = fl(u * inv_w)
 * The bin: t NaN: invalid += 1.  Otherwise bin = B/2 + floor(t), clamped to [0, B - 1], compared in
 * double before any conversion, so that +-inf saturate.  Zero is always a bin line, and u >= 0, -0.0
 * included, lands in the upper half for every extent.
 * g: device double[N], the caller's: the host forms g[k] = w_k / step_k^2, step_k the level spacing of
 * subcarrier k's LUT and w_k a weight, so that the unit is the squared minimum distance of the
 * subcarrier's own constellation.  inv_w = B / (2 L) for an extent L.  The library sees neither w nor L.
 * hist: device uint64[20][2][B] followed by one word `invalid`, 40 B + 1 words, accumulated and
 * never zeroed by the library.  row = (b/2)(b/2 - 1) + i: rows 0-1 for 4-QAM, 2-5 for 16-QAM, 6-11 for 64-QAM,
 * 12-19 for 256-QAM; the second index is the transmitted bit: hist[(row * 2 + tx bit) * B + bin] += 1.
 * Which bits count: exactly the bits counters[0] compares -- the n_valid_bits mask and the adaptive
 * partial-byte masking of ofdm_rx_frames -- of the subcarriers in [k_lo, k_hi).  Order-0 subcarriers carry
 * nothing.  The sum over the record equals the compared bits in range.  Integers only: the record is the
 * same for any grid, batching, split over calls or ranks, as long as every call takes the same form.
 * OFDM_E_INVALID, before any launch: what ofdm_rx refuses; hist or g NULL; bins odd or outside
 *   [2, OFDM_MAX_SOFT_BINS = 256]; inv_w not finite and positive; a range that is not
 *   0 <= k_lo < k_hi <= N; a plan with a non-separable (PSK) LUT or an order above 256 (not built); a
 *   layout that, with the histogram (160 B bytes), does not fit the 160 KB of LDS of a compute unit.
 *   n_sym = 0: an empty call.
 * Kernels (k_rx_soft), routed as ofdm_rx_density's: the complex128 bench shapes with throughput streams
 * and z_out == NULL run their throughput receiver's form, every other call the generic kernel's -- a call
 * with z_out != NULL also when z_keep is 0.  Everything else -- arguments, counters, z_out / z_keep -- is
 * ofdm_rx's.
 */
int ofdm_rx_soft(ofdm_plan_t plan, void* stream, const void* y, const double* nr, const double* ni,
                 uint64_t seed, const ofdm_stats* stats, int64_t total_samples, double snr_db,
                 int32_t noise_on, const uint8_t* bits, int64_t sym0, int64_t n_sym,
                 int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                 const double* g, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi, uint64_t* hist);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_HIP_SOFT_H */
