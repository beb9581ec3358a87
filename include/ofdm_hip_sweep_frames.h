/*
 * ofdm_hip_sweep_frames.h -- an extension header of libofdm_hip's C ABI (include/ofdm_hip.h, ABI 6): the
 * one-pass SNR sweep receiver with the per-frame error record of every point.  The entry point lives in
 * the same library; ofdm_hip.h, its types, its constants and every entry point it declares are as they were.
 */
#ifndef OFDM_HIP_SWEEP_FRAMES_H
#define OFDM_HIP_SWEEP_FRAMES_H

#include "ofdm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ofdm_rx_sweep with the per-frame error record of every point (an entry point added to ABI 6: nothing
 * of the version's existing interface, include/ofdm_hip.h, changes, so the number stands): the frame
 * error rate against SNR from one transmit, as ofdm_rx_sweep gives the BER against SNR.
 *
 * frames: device uint64[n_snr][n_frames][2], point-major (a list split over several calls takes the
 * contiguous slices frames[k0:k1]), accumulated and never zeroed by the library.  A frame is
 * F = frame_len >= 1 consecutive GLOBAL OFDM symbols, as ofdm_rx_frames'.  For every symbol s of the call
 * and every point k,
 *   frames[k][floor(s / F)][j] += exactly what ofdm_rx_frames(..., snr_db[k], noise_on = 1, bits = NULL,
 *                                 ..., frame_len = F) adds for that symbol
 * -- the symbol's share of counters[k][j] of ofdm_rx_sweep, under the same n_valid_bits and adaptive
 * partial-byte masking.  Everything is integer, so
 *   the sum over f of frames[k][f][j] over a call equals that call's increment of counters[k][j], and
 *   the record does not depend on the grid, the batching, the rank count, the order of the points, how a
 *   long list is split into calls, or whether a frame straddles any of those.
 * OFDM_E_INVALID, before any launch: what ofdm_rx_sweep refuses; frames == NULL; frame_len < 1;
 *   n_frames < 1; floor((sym0 + n_sym - 1) / frame_len) >= n_frames (the record is too short for the
 *   call's last symbol); n_sym above 2^31 (one call); sym0 + n_sym > OFDM_MAX_SYMBOLS.  n_sym = 0: an
 *   empty call.
 * Kernels (k_rx_sweep_frames), routed as ofdm_rx_sweep's: the complex128 cyclic-prefix OFDM fixed-QAM
 * bench shapes their throughput form, every other plan the generic one; the record needs no LDS.
 * Everything else -- arguments, counters -- is ofdm_rx_sweep's.
 */
int ofdm_rx_sweep_frames(ofdm_plan_t plan, void* stream, const void* y, uint64_t seed, const ofdm_stats* stats,
                         int64_t total_samples, const double* snr_db, int32_t n_snr, int64_t sym0,
                         int64_t n_sym, int64_t n_valid_bits, uint64_t* counters, int64_t frame_len,
                         int64_t n_frames, uint64_t* frames);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_HIP_SWEEP_FRAMES_H */
