/*
 * ofdm_hip.h -- C ABI of libofdm_hip.so, the MI355X (gfx950) implementation of the
 * per-symbol OFDM modem path of JomarJunior/ofdm-based-systems.
 *
 * Boundary: the reference is pure Python/NumPy; its "operator" interfaces
 * (src/ofdm_based_systems/<pkg>/models.py ABCs) are called from
 * Simulation.run (simulation/models.py:214-818).  This library exports the
 * arithmetic those operators perform; the Python package
 * ofdm-based-systems_amd/ofdm_based_systems mirrors the reference API and calls
 * these entry points through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every buffer argument is a DEVICE pointer owned by the caller (PyTorch
 *    allocates it).  The library owns only plan-scoped constant tables and a
 *    small partial-sum workspace per stream the plan is used on.
 *  - Complex arrays are interleaved (re, im) in the plan's precision:
 *    OFDM_F32 -> float2 (complex64), OFDM_F64 -> double2 (complex128).
 *  - Every call is asynchronous on the given hipStream_t (NULL = default stream);
 *    no call synchronises the device.  One plan may be used on several streams
 *    whose work overlaps (the reductions keep one workspace per stream); it must
 *    not be used on the SAME stream from two host threads at once.
 *  - Return 0 on success, a negative OFDM_E* code on failure; the message is in
 *    ofdm_last_error() (thread-local).  Nothing throws across the ABI.
 *  - Bits are packed MSB-first in bytes (simulation/models.py:59-69,
 *    constellation/models.py:227-233).
 */
#ifndef OFDM_HIP_H
#define OFDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_ABI_VERSION 6

/* SNR points one ofdm_rx_sweep call takes (the kernels hold a noise table per point in LDS and the
 * points' SNRs in their arguments); a longer list is split into several calls over the same y. */
#define OFDM_MAX_SWEEP_POINTS 40

/* The supported symbol range: every entry point that takes sym0 and n_sym (ofdm_tx, ofdm_tx_clip,
 * ofdm_rx, ofdm_rx_profile, ofdm_rx_frames, ofdm_rx_density, ofdm_rx_sweep, the four ofdm_link*,
 * ofdm_papr and ofdm_hip_soft.h's receiver) returns OFDM_E_INVALID, before any launch, when sym0 + n_sym > OFDM_MAX_SYMBOLS.
 * The host and the kernels form global bit positions s * bps + offset in int64_t (the n_valid_bits
 * mask, the caller's bits and their byte count), s < sym0 + n_sym and bps the bits per OFDM symbol.
 * The largest plan has 4096 subcarriers of 12 bits (4096-QAM): bps <= 49152 < 2^16, and an offset
 * inside one symbol is below bps.  With s <= 2^46 every such value stays below 2^46 * 2^16 = 2^62,
 * a factor of two inside int64_t, so no product, sum or rounding up to bytes can wrap. */
#define OFDM_MAX_SYMBOLS ((int64_t)1 << 46)

#define OFDM_OK 0
#define OFDM_E_INVALID (-1)  /* bad argument / unsupported shape          */
#define OFDM_E_HIP (-2)      /* HIP runtime error                          */
#define OFDM_E_ALLOC (-3)    /* device allocation failed (plan creation)   */

enum ofdm_precision { OFDM_F32 = 0, OFDM_F64 = 1 };
/* equalization/models.py:22-68 */
enum ofdm_equalizer { OFDM_EQ_NONE = 0, OFDM_EQ_ZF = 1, OFDM_EQ_MMSE = 2 };

/* prefix/models.py:29-113 (NoPrefixScheme = OFDM_PREFIX_CYCLIC with cp = 0) */
enum ofdm_prefix { OFDM_PREFIX_CYCLIC = 0, OFDM_PREFIX_ZERO = 1 };
/* modulation/models.py:19-91: OFDMModulator / SingleCarrierOFDMModulator */
enum ofdm_modulator { OFDM_MOD_OFDM = 0, OFDM_MOD_SC = 1 };

typedef struct ofdm_plan_s* ofdm_plan_t;

/*
 * Plan descriptor.  One plan = one (N, prefix, channel, constellation, equaliser)
 * configuration, i.e. what Simulation.run builds once per SNR point
 * (simulation/models.py:248-275, :399-404) or what one operator object holds.
 */
typedef struct ofdm_desc {
    int32_t n_fft;       /* N = num_subcarriers, power of two in [1, 4096]        */
    int32_t cp;          /* guard length (IPrefixScheme.prefix_length)            */
    int32_t prefix;      /* enum ofdm_prefix: cyclic prefix or zero padding       */
    int32_t precision;   /* enum ofdm_precision                                   */
    int32_t equalizer;   /* enum ofdm_equalizer                                   */
    /* Constellations: a pool of LUTs (interleaved re/im doubles, exactly the
       reference's QAMConstellationMapper.constellation arrays) and, per
       subcarrier, which LUT it uses.  Fixed mode: one LUT, sc_lut == NULL.
       Adaptive mode (constellation/adaptive.py:16-91): n_luts LUTs and
       sc_lut[k] in [-1, n_luts) with -1 = inactive subcarrier (order 0).
       Orders are powers of two up to 4096 (12 bits per subcarrier: 1024- and 4096-QAM,
       PSK up to 4096 points).  The pool holds at most 512 entries while every order is
       <= 256, at most 8192 once an order is larger (the reference's QAM pool 4..4096 is
       5460).  Orders above 256 run with caller-supplied bits only (ofdm_tx / ofdm_rx). */
    int32_t n_luts;              /* 0 = no constellation in this plan, at most 8   */
    const int32_t* lut_orders;   /* [n_luts] orders (powers of two 2..4096)        */
    const double* lut_pool;      /* concatenated LUTs, sum(lut_orders) complex      */
    const int32_t* sc_lut;       /* [n_fft] or NULL                                 */
    /* Channel: raw CIR (h_raw).  The plan normalises it to unit power for the
       convolution (channel/models.py:37-44) and computes the equaliser response
       fft(h_raw, N) on the device (simulation/models.py:264). */
    int32_t n_taps;              /* 0 = no channel in this plan                     */
    const double* h_raw;         /* [n_taps] complex                                */
    /* Optional explicit equaliser response (IEqualizator(channel_frequency_response=H)),
       [n_fft] complex; overrides the response derived from h_raw. */
    const double* H;
    /* enum ofdm_modulator (ABI 2): the fused path's modulator (ofdm_tx / ofdm_rx). */
    int32_t modulator;
} ofdm_desc;

/*
 * Whole-stream statistics of the fused transmitter (ABI 3), one device record per run, zeroed
 * by the caller and accumulated by every ofdm_tx of the run.  The AWGN power is the mean of |y|^2
 * over the whole serial stream (noise/models.py:14); so that it -- and sigma -- does not depend on
 * how a run is batched or sharded over GPUs, the sum is kept EXACTLY: every lane's share of one
 * OFDM symbol is rounded once to 2^-40 fixed point and added as 32-bit limbs to 64-bit integers,
 * power_fx[0] + 2^32 power_fx[1] (units of 2^-40).  Records of several ranks combine by adding
 * the limbs (any order: integer arithmetic), then power_fx[1] += power_fx[0] >> 32,
 * power_fx[0] &= 2^32 - 1, power_sum = power_fx[1] 2^-8 + power_fx[0] 2^-40 (IEEE double).
 */
typedef struct ofdm_stats {
    double power_sum;     /* sum |y|^2 over all N+cp samples, = value of power_fx            */
    double x_power_sum;   /* sum |x|^2 over the modulated samples incl. the guard          */
    double x_peak;        /* max |x|^2 (simulation/models.py:519-522)                       */
    int64_t power_fx[2];  /* sum |y|^2 in 2^-40 fixed point, 32-bit limbs (see above)       */
} ofdm_stats;

typedef struct ofdm_plan_info {
    int32_t n_fft, cp, precision, equalizer, n_taps;
    int32_t bits_per_ofdm_symbol; /* sum of bits over active subcarriers            */
    int32_t bits_per_subcarrier;  /* uniform b in fixed mode, -1 in adaptive mode   */
    int32_t adaptive;
    double channel_gain_mean;     /* mean |H|^2 (equalization/models.py:46)          */
} ofdm_plan_info;

int ofdm_abi_version(void);
const char* ofdm_last_error(void);

int ofdm_plan_create(ofdm_plan_t* plan, const ofdm_desc* desc, void* stream);
int ofdm_plan_destroy(ofdm_plan_t plan);
int ofdm_plan_get_info(ofdm_plan_t plan, ofdm_plan_info* info);

/* The plan's channel response H = fft(h_raw, N) (or the explicit desc.H) and, if
   gains != NULL, |H|^2 (ChannelModel.get_frequency_response / get_gains,
   channel/models.py:26-35).  H: device complex128 [N]; gains: device double [N]. */
int ofdm_plan_response(ofdm_plan_t plan, void* stream, double* H, double* gains);

/* ---------------------------------------------------------------- operators
 * Drop-in arithmetic for the reference's operator objects.                    */

/* In-place batched FFT of `batch` contiguous rows of N (norm="ortho").
   Replaces np.fft.fft / np.fft.ifft(axis=1, norm="ortho") in
   modulation/models.py:32 and :46-48. */
int ofdm_fft(ofdm_plan_t plan, void* stream, void* data, int64_t batch, int32_t inverse);

/* QAMConstellationMapper.encode (constellation/models.py:220-249) and
   AdaptiveConstellationMapper.encode (constellation/adaptive.py:130-201):
   n_bytes packed bytes -> n_out complex symbols.  Fixed mode: symbol e uses bits
   [e*b, e*b+b), bits past the input are zero (padding :235-237).  Adaptive mode:
   n_out = S*N, subcarrier k of OFDM symbol s uses bits at s*sum(b)+off[k]; inactive
   subcarriers are 0+0j. */
int ofdm_map(ofdm_plan_t plan, void* stream, const uint8_t* bytes, int64_t n_bytes,
             int64_t n_out, void* symbols);

/* QAMConstellationMapper.decode (constellation/models.py:251-295): nearest LUT point
   by brute-force |z - C_m| argmin (first index on ties, NNClassifier :19-27), bits
   packed MSB-first; fixed mode writes ceil(n*b/8) bytes (tail zero-padded), adaptive
   mode floor(S*sum(b)/8) bytes (constellation/adaptive.py:257-265).
   Zero components (the per-axis path of sides 32 and 64, ofdm_demap_count and the fused receivers,
   which round a level coordinate where this searches): a real or imaginary part that is exactly
   +-0 lies halfway between the two central levels of a square QAM, and 0+0j ties between its four
   central points -- what an MMSE equaliser puts out on a subcarrier whose channel response is
   exactly zero, in every OFDM symbol.  The decision there is the argmin's: the first index, which
   for the reference's LUTs is the lower central level on I and the upper one on Q.  Every plan reads
   the two levels off each LUT when it is created (the levels of LUT[argmin |C_m|]); they are not
   left to how lev0 / step rounds. */
int ofdm_demap(ofdm_plan_t plan, void* stream, const void* z, int64_t n, uint8_t* bytes);

/* QAMConstellationMapper.decode (constellation/models.py:251-295) or
   AdaptiveConstellationMapper.decode (constellation/adaptive.py:203-265) followed by
   Simulation.run's error count (simulation/models.py:596-606), fused: Z is (n_sym, N)
   equalised symbols in the plan precision, tx_bits the packed bits of those symbols (OFDM
   symbol s from bit s*bits_per_ofdm_symbol, MSB first).  Nearest point per subcarrier as
   ofdm_demap; counters[0] += bit errors (every bit in fixed mode, whole bytes of the run in
   adaptive mode, as the reference's decode), counters[1] += symbol errors.  counters: 2 device
   uint64 accumulated atomically. */
int ofdm_demap_count(ofdm_plan_t plan, void* stream, const void* Z, const uint8_t* tx_bits,
                     int64_t n_sym, uint64_t* counters);

/* NNClassifier.classify (constellation/models.py:19-27) for an arbitrary LUT of M
   complex128 points: idx[i] = argmin_m |z_i - lut_m| (first on ties).  z is complex128. */
int ofdm_nn_classify(void* stream, const double* lut, int32_t m, const void* z, int64_t n,
                     int64_t* idx);

/* Throughput-mode noise radius (ABI 4; ABI 5: stream version 3, the radius takes the whole word):
   radius[i] = sqrt(32 - log2(float(words[i] | 1))),
   evaluated exactly as the fused receivers evaluate it for every lane word (the float32 hardware
   log2 / square root: the one step of the stream definition, csrc/ofdm_device.hpp noise_radius,
   that IEEE arithmetic does not pin).  AWGNoiseModel.add_noise's Gaussian (noise/models.py:19-21)
   in throughput mode is sigma sqrt(2 ln 2) radius (cos, sin)(phase); the checker
   (oracle/philox_streams.py) takes these radii to restate the receivers' noise bit for bit.
   words: device uint32 [n]; radius: device float [n]. */
int ofdm_noise_radius(void* stream, const uint32_t* words, int64_t n, float* radius);

/* OFDMModulator.modulate (modulation/models.py:27-39): x[s] = [cp | ifft(X[s], ortho)]
   (zero padding: [ifft(X[s], ortho) | 0...0]), X is (n_sym, N), x is (n_sym, N+cp). */
int ofdm_modulate(ofdm_plan_t plan, void* stream, const void* X, int64_t n_sym, void* x);

/* OFDMModulator.demodulate (modulation/models.py:41-55): strip cp (zero padding: fold
   the tail onto the head, prefix/models.py:74-101), fft(ortho), per-row equalise
   (equalization/models.py:22-68).  yt is (n_sym, N+cp), Z (n_sym, N). */
int ofdm_demodulate(ofdm_plan_t plan, void* stream, const void* yt, int64_t n_sym,
                    double snr_db, void* Z);

/* IEqualizator.equalize applied to n_rows rows of N (equalization/models.py:22-68). */
int ofdm_equalize(ofdm_plan_t plan, void* stream, const void* Y, int64_t n_rows,
                  double snr_db, void* Z);

/* ChannelModel.transmit convolution (channel/models.py:46-55): y = conv(s, h/|h|)[:len].
   If power_sum != NULL, *power_sum (device double) += sum |y|^2. */
int ofdm_channel(ofdm_plan_t plan, void* stream, const void* s, int64_t len, void* y,
                 double* power_sum);

/* AWGNoiseModel.add_noise (noise/models.py:13-22) with caller-supplied standard normals
   (the reference's legacy-RNG draws, real array first):
   y += sqrt((power_sum/len) / 10^(snr/10) / 2) * (nr + j*ni).  power_sum is a device
   double holding sum |y|^2 over the len samples (from ofdm_channel or ofdm_power). */
int ofdm_awgn(ofdm_plan_t plan, void* stream, void* y, int64_t len, const double* nr,
              const double* ni, const double* power_sum, double snr_db);

/* *power_sum += sum |y|^2 over len samples (device double). */
int ofdm_power(ofdm_plan_t plan, void* stream, const void* y, int64_t len, double* power_sum);

/* ---------------------------------------------------------------- fused hot path
 * Simulation.run's data path (simulation/models.py:454-606) in two kernels.
 *
 * Bit source: `bits` != NULL -> packed tx bytes of the WHOLE run (OFDM symbol s
 * starts at bit s*bits_per_ofdm_symbol), e.g. the reference's PCG64 bytes
 * (parity mode).  bits == NULL -> throughput mode: bits and noise from the
 * counter-based lane streams keyed by (seed, global symbol) (stream version 3 since ABI 5:
 * Philox4x32-10 seeding MWC64X; definition in csrc/ofdm_device.hpp, restated in
 * oracle/philox_streams.py).  Caller bits on the bench shapes (complex128 OFDM, cyclic prefix,
 * 64-QAM at N = 1024, adaptive square-QAM loading at N = 2048 or 256-QAM at N = 4096) run the
 * throughput kernels with the bit -- and in
 * ofdm_rx, with nr/ni and no z_out, the noise -- source swapped; other shapes the generic kernel.  n_sym = 0 is an empty call (returns 0, launches nothing).
 * The throughput streams give each subcarrier one byte, so a plan with more than 8 bits on a
 * subcarrier (orders above 256) takes caller bits only: bits == NULL returns OFDM_E_INVALID.
 * A shape whose kernel layout does not fit a compute unit's LDS returns OFDM_E_INVALID naming
 * the shape (every shape a plan accepts up to N = 4096, 32 taps, 4096-QAM fits).
 *
 * ofdm_tx: for global OFDM symbols [sym0, sym0+n_sym): map -> IFFT(ortho) (OFDM) or
 *   nothing (single carrier) -> cyclic prefix or zero guard -> linear convolution with
 *   the normalised CIR across symbol boundaries (channel/models.py:52-55).  Writes the
 *   channel-output samples of each symbol to y[(s-sym0)*ystride + n], ystride = N (the
 *   post-prefix samples) or N + cp with zero padding (all samples: the receiver
 *   overlap-adds the guard); y may be NULL (power pass only).  Accumulates into the device
 *   record stats (ofdm_stats): sum|y|^2 over all N+cp samples (noise/models.py:14) in exact
 *   fixed point, sum|x|^2 and max|x|^2 over the modulated samples incl. the guard
 *   (simulation/models.py:519-522).
 *
 * ofdm_rx: adds AWGN with sigma^2 = (stats->power_sum/total_samples)/10^(snr/10) (noise_on=0:
 *   no noise), strips the prefix (or overlap-adds the zero guard, prefix/models.py:69-101),
 *   FFT(ortho), equalises (MMSE noise variance per OFDM symbol, equalization/models.py:
 *   39-49), IFFT(ortho) for single carrier, decides the nearest constellation point
 *   (per-axis slicer for square QAM, brute force over the LUT otherwise) and compares
 *   against the tx bits: counters[0] += bit errors over global bit positions
 *   < n_valid_bits, counters[1] += symbol errors (simulation/models.py:596-606).
 *   Noise: nr/ni != NULL -> the reference's normals for the whole serial stream
 *   (sample s*(N+cp)+m); NULL -> the throughput-mode lane streams, Box-Muller.
 *   z_out (optional): the equalised symbols of the first z_keep OFDM symbols of this
 *   call, (z_keep, N) complex -- the results' received_symbols (simulation/models.py:618).
 *   Null bins: a plan whose channel response is exactly 0 on a subcarrier (taps such as [1, -1])
 *   is a legal plan.  Under MMSE the equalised symbol there is exactly 0 in every OFDM symbol and
 *   decides the first of the four central points, as the reference's argmin does (see ofdm_demap:
 *   the zero-component rule); such a plan's receivers -- ofdm_rx and every ofdm_rx_* form -- run
 *   the generic kernel, whose slicer applies the rule, whatever the shape and the streams.  Under
 *   ZF the reference divides by 1e-10 there: the symbol is the noise times 1e10, decided by its
 *   signs (the level coordinate is clamped before it is converted to an integer).
 */
int ofdm_tx(ofdm_plan_t plan, void* stream, const uint8_t* bits, uint64_t seed, int64_t sym0,
            int64_t n_sym, void* y, ofdm_stats* stats);

int ofdm_rx(ofdm_plan_t plan, void* stream, const void* y, const double* nr, const double* ni,
            uint64_t seed, const ofdm_stats* stats, int64_t total_samples, double snr_db,
            int32_t noise_on, const uint8_t* bits, int64_t sym0, int64_t n_sym,
            int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep);

/*
 * ofdm_rx with a per-subcarrier profile of the run (ABI 6).  The reference returns every equalised
 * symbol as received_symbols and compares the decoded bits against the transmitted ones
 * (simulation/models.py:596-618); its per-subcarrier views are computed from that array.  Here the
 * per-subcarrier sums are accumulated on the device, where the decisions are made.
 *
 * profile: device int64[5][N], zeroed by the caller and accumulated by every call of a run (of
 * every batch; the records of several ranks add as integers).  Row r of subcarrier k:
 *   0  bit errors:    subcarrier k's share of counters[0] (the same n_valid_bits and adaptive
 *                     partial-byte masking); sum over k = this call's counters[0] increment, exactly
 *   1  symbol errors: its share of counters[1], the same invariant
 *   2, 3  error-vector power sum over the symbols of min(|z - c|^2, 2^20) as 32-bit limbs in units of
 *                     2^-40, the format of ofdm_stats.power_fx: value = row3 2^-8 + row2 2^-40 after
 *                     row3 += row2 >> 32, row2 &= 2^32 - 1.  z is the equalised symbol as z_out
 *                     reports it (MMSE scale applied, after the IFFT for single carrier), c the
 *                     transmitted point of the plan's LUT; each sample is rounded once to 2^-40
 *   4  clipped:       samples whose |z - c|^2 reached the cap 2^20 or was not finite (ZF on a null bin)
 * Inactive subcarriers (adaptive order 0) stay zero in every row.  Integer accumulation throughout:
 * the record is identical for any batching, grid and rank count.
 * Kernels: the complex128 bench shapes (cyclic-prefix OFDM; 64-QAM at N = 1024, adaptive square-QAM
 * loading at N = 2048, 256-QAM at N = 4096) with throughput streams (bits == NULL, nr == NULL) and no
 * z_out run their throughput receiver's k_rx_prof instantiation; every other call the generic
 * kernel's.  Everything else -- arguments, counters, z_out / z_keep -- is ofdm_rx's.
 */
int ofdm_rx_profile(ofdm_plan_t plan, void* stream, const void* y, const double* nr, const double* ni,
                    uint64_t seed, const ofdm_stats* stats, int64_t total_samples, double snr_db,
                    int32_t noise_on, const uint8_t* bits, int64_t sym0, int64_t n_sym,
                    int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                    int64_t* profile);

/*
 * ofdm_rx with a per-frame error record of the run (an entry point added to ABI 6: nothing of the
 * version's existing interface changes, so the number stands): when the errors fall, where
 * ofdm_rx_profile says where.  From it come the frame (packet) error rate, a standard error on the BER
 * that holds when bit errors are not independent, and the distribution of errors per frame.
 *
 * A frame is F = frame_len >= 1 consecutive GLOBAL OFDM symbols: symbol s belongs to frame
 * f = floor(s / F), whatever the call's sym0.
 * frames: device uint64[n_frames][2], accumulated and never zeroed by the library.  For every symbol s
 * of the call,
 *   frames[f][0] += the bit errors of symbol s: exactly that symbol's share of counters[0], under the
 *                   same n_valid_bits and adaptive partial-byte masking
 *   frames[f][1] += its share of counters[1].
 * So the sum over f of frames[f][j] over a call equals that call's increment of counters[j], exactly;
 * and, the additions being integer, the record does not depend on the grid, the batching, the split of
 * a run over calls or ranks, or whether a frame straddles any of those.
 * OFDM_E_INVALID, before any launch: what ofdm_rx refuses; frames == NULL; frame_len < 1; n_frames < 1;
 *   floor((sym0 + n_sym - 1) / frame_len) >= n_frames (the record is too short for the call's last
 *   symbol); n_sym above 2^31 (one call).  n_sym = 0: an empty call.
 * Kernels (k_rx_frames): the complex128 bench shapes (cyclic-prefix OFDM; 64-QAM at N = 1024, adaptive
 * square-QAM loading at N = 2048, 256-QAM at N = 4096) with throughput streams (bits == NULL,
 * nr == NULL) and no z_out run their throughput receiver's form, in ofdm_rx's own workgroup shape;
 * every other call the generic kernel's.  Everything else -- arguments, counters, z_out / z_keep -- is
 * ofdm_rx's.
 */
int ofdm_rx_frames(ofdm_plan_t plan, void* stream, const void* y, const double* nr, const double* ni,
                   uint64_t seed, const ofdm_stats* stats, int64_t total_samples, double snr_db,
                   int32_t noise_on, const uint8_t* bits, int64_t sym0, int64_t n_sym,
                   int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                   int64_t frame_len, int64_t n_frames, uint64_t* frames);

/* Bins per axis of ofdm_rx_density's grid at most: the kernel's histogram is G * G 32-bit bins in LDS,
 * 64 KB at 128. */
#define OFDM_MAX_DENSITY_BINS 128

/*
 * ofdm_rx with a constellation-density record of the run (an entry point added to ABI 6: nothing of the
 * version's existing interface changes, so the number stands): where the received points fall in the
 * I/Q plane, every equalised point of the call binned into a G x G grid over a square.
 *
 * The value binned: for every OFDM symbol of the call and every active element, the equalised symbol v
 * -- the value the received-symbol tap (z_out) stores for that element, in the plan's precision.  The
 * throughput receivers, which fold the MMSE scale and 1/sqrt(N) into the slicer, bin the point
 * ofdm_rx_profile forms for its error vector (the unscaled equaliser output times that scale).  An
 * adaptive plan's order-0 subcarriers carry no point and are not binned; SC-OFDM and zero padding bin
 * what their tap would store.
 * Subcarrier range [k_lo, k_hi): only elements whose subcarrier index k lies in it are binned (the whole
 * symbol: 0, N); elements outside it count nowhere.
 * The grid: G = bins per axis, 1 <= G <= OFDM_MAX_DENSITY_BINS = 128, given by two doubles the host forms in double from an
 * extent L: lo = -L and inv_w = G / (2 L).  The library never sees L.
 * The index is taken in double in both precisions (a complex64 component is widened first, which is
 * exact).  Per axis t = (c - lo) * inv_w, one rounded subtraction and one rounded multiplication, never
 * contracted into an FMA: the same two IEEE operations on the same c give the same t anywhere.  The
 * point is inside iff 0 <= t < G on both axes (a NaN or an infinity fails the comparison: a ZF point on
 * a null bin is outside).  Inside: hist[iy * G + ix] += 1, ix = (int) t of the real part, iy of the
 * imaginary part.  Otherwise hist[G * G] += 1, the `outside` count.
 * hist: device uint64[G * G + 1], accumulated and never zeroed by the library.  Integers only; a point's
 * v is a function of (plan, seed or caller streams, symbol) in a given kernel form, so the record is the
 * same for any grid, batching, split of a run over calls (sym0) or ranks, as long as every call of the
 * run takes the same form.
 * OFDM_E_INVALID, before any launch: what ofdm_rx refuses; hist == NULL; bins outside [1, 128]; lo or
 *   inv_w not finite, or inv_w <= 0; a range that is not 0 <= k_lo < k_hi <= N; a layout that, with the
 *   histogram (4 G^2 bytes), does not fit the 160 KB of LDS of a compute unit.  n_sym = 0: an empty call.
 * Kernels (k_rx_dens), routed as ofdm_rx_profile's: the complex128 bench shapes (cyclic-prefix OFDM;
 * 64-QAM at N = 1024, adaptive square-QAM loading at N = 2048, 256-QAM at N = 4096) with throughput
 * streams (bits == NULL, nr == NULL) and z_out == NULL run their throughput receiver's form; every other
 * call the generic kernel's -- a call with z_out != NULL also when z_keep is 0, so that a run with a tap
 * can hold one form over all its calls.  Everything else -- arguments, counters, z_out / z_keep -- is
 * ofdm_rx's.
 */
int ofdm_rx_density(ofdm_plan_t plan, void* stream, const void* y, const double* nr, const double* ni,
                    uint64_t seed, const ofdm_stats* stats, int64_t total_samples, double snr_db,
                    int32_t noise_on, const uint8_t* bits, int64_t sym0, int64_t n_sym,
                    int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                    double lo, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi, uint64_t* hist);

/* The receiver with a soft-decision record of the run, ofdm_rx_soft -- for every compared bit the max-log
 * distance difference, binned into a histogram conditioned on the transmitted bit -- is declared in the
 * extension header ofdm_hip_soft.h (an entry point added to ABI 6 in the same library; nothing here changes). */

/*
 * The one-pass SNR sweep receiver (an entry point added to ABI 6: nothing of the version's existing
 * interface changes, so the number stands): ofdm_rx of the same channel samples at n_snr SNR points in
 * one launch.  The transmitted stream, the tx bits and the noise words of throughput mode depend on
 * (seed, symbol, N) only; the SNR enters through sigma and the MMSE noise variance.  So every symbol
 * is read once, its lane block and noise words are drawn once, and per point the noise is scaled by
 * the point's phase table and the symbol goes through ofdm_rx's FFT, equaliser, slicer and count:
 * counters[2 k], counters[2 k + 1] += what ofdm_rx(..., snr_db[k], noise_on = 1, bits = NULL, ...)
 * adds to its counters[0], counters[1] -- the same bits, noise words, sigma (from stats->power_sum /
 * total_samples) and arithmetic per received sample; integer accumulation, so the counts do not
 * depend on the grid, the batching, the rank count, the order of the points or how a list is split
 * over calls.  The points share their noise realisation (common random numbers).
 *
 * Throughput streams only: no bits, nr / ni, z_out or profile; noise is always on.
 * snr_db: HOST array [n_snr] -- the one host-side array of this ABI -- copied at the call (it may be
 *   freed or changed once the call returns).
 * counters: device uint64 [n_snr][2], accumulated.
 * OFDM_E_INVALID, before any launch: n_snr outside [1, OFDM_MAX_SWEEP_POINTS], a non-finite SNR, a
 *   plan with more than 8 bits on a subcarrier (as ofdm_rx with bits == NULL).  n_sym = 0: an empty call.
 * Kernels (k_rx_sweep): the complex128 cyclic-prefix OFDM fixed-QAM bench shapes (64-QAM at N = 1024,
 * 256-QAM at N = 4096) their throughput receiver's form, which keeps y and the noise radii in
 * registers across the points; every other plan the generic receiver's, which reloads y and replays
 * the lane generator per point.  A plan per point (adaptive loading re-derived per SNR) is not a sweep.
 */
int ofdm_rx_sweep(ofdm_plan_t plan, void* stream, const void* y, uint64_t seed, const ofdm_stats* stats,
                  int64_t total_samples, const double* snr_db, int32_t n_snr, int64_t sym0, int64_t n_sym,
                  int64_t n_valid_bits, uint64_t* counters);

/* ofdm_rx_sweep with the per-frame error record of every point: include/ofdm_hip_sweep_frames.h, an
 * extension header of this ABI version (it declares one more entry point of the same library). */

/* The fused link: transmit and receive symbols [sym0, sym0 + n_sym) in one kernel, without the kept
 * channel samples ever leaving the registers -- adds to `counters` what ofdm_tx(plan, stream, NULL, seed,
 * sym0, n_sym, y, ...) into a buffer followed by ofdm_rx(plan, stream, y, NULL, NULL, seed, stats,
 * total_samples, snr_db, noise_on, NULL, sym0, n_sym, n_valid_bits, counters, NULL, 0) of that buffer
 * would add.  In throughput mode y is a pure function of (seed, symbol): each wave maps its symbol's
 * lane block through the LUT and the IFFT exactly as the transmitter does -- the same code, the same
 * operation order, so the values are the ones ofdm_tx would have stored -- and receives them in place
 * (noise, FFT, slicer, count: ofdm_rx's arithmetic), the lane block drawn once for both.  Integer
 * accumulation: the counts do not depend on the grid, the batching or the rank count.
 *
 * It writes no statistics: `stats` is read (power_sum scales the noise, as in ofdm_rx) and must hold the
 * whole stream's record, e.g. from a power pass ofdm_tx(..., y = NULL, stats) over every symbol (and,
 * with several ranks, their reduction).
 * A fused form exists for: complex128, n_fft 1024, fixed 64-QAM, OFDM with a cyclic prefix or none, a
 * one-tap (flat) channel, OFDM_EQ_NONE (the bench's config b).  Any other plan, or an n_valid_bits
 * short of all the call's bits ((sym0 + n_sym) * bits per OFDM symbol; the fixed-order receivers
 * compare every bit), returns OFDM_E_INVALID with the reason in ofdm_last_error(), before any launch:
 * there is no fall-back to another path.  n_sym = 0: an empty call.
 * counters: device uint64 [2], accumulated.
 * The float32 noise screen with the sparse slicer (ofdm_link_sparse below) runs in its automatic mode;
 * the counts are the same in every mode, and with the other screens (ofdm_link_nscreen,
 * ofdm_link_screen).
 */
int ofdm_link(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
              double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
              uint64_t* counters);

/* Modes of the fused link's float32 screens. */
#define OFDM_LINK_SCREEN_AUTO 0   /* the kernel decides from sigma and the level spacing */
#define OFDM_LINK_SCREEN_OFF 1    /* every symbol in complex128: the unscreened kernel (for A/B) */
#define OFDM_LINK_SCREEN_FORCED 2 /* every symbol screened, whatever the SNR */

/*
 * The fused link with the two-transform float32 screen, its mode and counts (an entry point added to
 * ABI 6: nothing of the version's existing interface changes, so the number stands).  ofdm_link itself
 * runs the noise screen (ofdm_link_nscreen below), which is cheaper and decides more symbols; this entry
 * stays for A/B runs and diagnosis.  The fused kernel reports integer decisions only,
 * and a decision needs complex128 only when the received point lies within rounding distance of a
 * slicer boundary.  A screened wave runs its symbol in float32 first and proves, per element and axis,
 * that the level coordinate is further from every decision boundary than a rigorous bound on the
 * distance between the float32 and the float64 coordinate of this symbol; if any element fails, the wave
 * redoes the whole symbol in complex128.  Either way the decisions are the complex128 ones: `counters`
 * receives exactly what ofdm_link's complex128 arithmetic adds, in every mode and for any share redone.
 * Automatic mode screens when the noise is off or the expected share of undecided symbols is small
 * (64-QAM: from about 22 dB up), a decision made once per launch from sigma and the level spacing.
 * mode: OFDM_LINK_SCREEN_AUTO, _OFF or _FORCED; anything else is OFDM_E_INVALID.
 * screen_counts: optional device uint64 [2], accumulated: symbols screened, and symbols of those redone
 *   in complex128 (both stay as they are when the screen is off).
 * Everything else -- arguments, refusals, no fall-back -- as ofdm_link.
 */
int ofdm_link_screen(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats,
                     int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym,
                     int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* screen_counts);

/*
 * The fused link with the noise screen, every quad sliced, its mode and counts (an entry point added to
 * ABI 6: nothing of the version's existing interface changes, so the number stands).  ofdm_link itself
 * runs this screen with the sparse slicer (ofdm_link_sparse below); this entry stays as its A/B
 * baseline.  The fused form's channel is one tap
 * folded into the constellation table and nothing is done to the prefix, so the spectrum the slicer
 * sees is, in exact arithmetic, N times the table entry of each subcarrier plus the unnormalised FFT of
 * the symbol's noise.  A screened wave transforms the noise alone in float32 (one transform, where
 * ofdm_link_screen runs two), adds the table point, and proves per element and axis that the level
 * coordinate is further from every decision boundary than a rigorous bound on its distance from the
 * complex128 coordinate -- a bound that scales with the noise, not with the signal; if any element
 * fails, the wave redoes the whole symbol in complex128.  `counters` receives exactly what ofdm_link's
 * complex128 arithmetic adds, in every mode and for any share redone.
 * Automatic mode screens when the noise is off or the expected share of undecided symbols is small
 * enough to pay, a decision made once per launch (ofdm_link's rule for screening).
 * mode: OFDM_LINK_SCREEN_AUTO, _OFF (the unscreened kernel) or _FORCED; anything else is OFDM_E_INVALID.
 * screen_counts: optional device uint64 [2], accumulated: symbols screened, and symbols of those redone
 *   in complex128 (both stay as they are when the screen is off).
 * Everything else -- arguments, refusals, no fall-back -- as ofdm_link.
 */
int ofdm_link_nscreen(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats,
                      int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym,
                      int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* screen_counts);

/*
 * ofdm_link with the sparse slicer's mode and counts (an entry point added to ABI 6: nothing of the
 * version's existing interface changes, so the number stands).  The kernel is the noise screen
 * (ofdm_link_nscreen above) up to the symbol's bound.  Before the table point is added, a screened wave
 * holds the float32 transform of the noise alone, and for each quad -- elements 4q .. 4q+3 of every lane,
 * 512 components of the wave -- it takes the largest modulus of a component and compares it with a
 * per-symbol threshold T.  T is chosen so that a quad with no component over it provably gives the
 * transmitted levels and a margin inside the screen's: the add, the slicer and the counts are skipped
 * for it, and run unchanged for every other quad.  The counters, the set of symbols redone in complex128
 * and the screen's two counts are ofdm_link_nscreen's for every input.
 * Automatic mode (what ofdm_link runs) decides once per launch, from sigma and the level spacing, both
 * whether to screen (the noise screen's rule) and whether to test the quads or slice them all (when
 * the expected number of components over T per quad is too large for the test to pay).
 * mode: OFDM_LINK_SCREEN_AUTO; _OFF (the noise screen itself in its automatic mode, sparse_counts left
 *   as they are); _FORCED (every symbol screened and every quad tested, whatever the SNR); anything else
 *   is OFDM_E_INVALID.
 * sparse_counts: optional device uint64 [4], accumulated: symbols screened, symbols of those redone in
 *   complex128, quads tested, and quads of those sliced (a launch that slices every quad tests none).
 * Everything else -- arguments, refusals, no fall-back -- as ofdm_link.
 */
int ofdm_link_sparse(ofdm_plan_t plan, void* stream, uint64_t seed, const ofdm_stats* stats,
                     int64_t total_samples, double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym,
                     int64_t n_valid_bits, uint64_t* counters, int32_t mode, uint64_t* sparse_counts);

/* Edges one ofdm_papr call takes (the kernels hold them, and a bin per edge plus one, in LDS). */
#define OFDM_MAX_PAPR_EDGES 128

/*
 * The per-symbol PAPR histogram (an entry point added to ABI 6: nothing of the version's existing
 * interface changes, so the number stands).  Take global OFDM symbol s.  Its modulated samples are
 * x_s[0 .. n), n = N + cp: what ofdm_tx's PAPR statistics see -- after the map, and after the
 * IFFT(ortho) for OFDM (single carrier has no transform); including the cyclic prefix, or the zero
 * guard, whose zeros count in n and add no power; before the channel.
 * peak_s = max |x|^2, sum_s = sum |x|^2: lane partials in the arithmetic precision R, reduced over the
 * symbol's lanes in R.  Then
 *  - given edges[0 .. K) as linear ratios, strictly increasing, the symbol's bin is
 *    j = #{ i : (double)peak_s * (double)n >= edges[i] * (double)sum_s }, the comparison evaluated in
 *    double in both precisions; no logarithm is taken on the device;
 *  - hist[j] += 1; bin 0 lies below the first edge and bin K at or above the last;
 *  - a symbol with sum_s = 0 lands in bin K (0 >= 0 holds): the reference's inf;
 *  - each symbol's pair is computed by the same lanes in the same order for any grid and the counts are
 *    integers, so the histogram is identical for any grid, batching, sym0 split and rank count.
 *
 * bits: as in ofdm_tx -- the caller's bytes of the whole run (reference mode), or NULL (Philox stream
 *   version 3).
 * edges: HOST array [n_edges] -- the second host-side array of this ABI, after snr_db -- copied at the
 *   call into the kernel's arguments (it may be freed or changed once the call returns).
 * hist: device uint64 [n_edges + 1], accumulated, not zeroed.
 * sym_out: optional device double [sym_keep][2]: (peak_s, sum_s) of the first min(sym_keep, n_sym)
 *   symbols of the call, widened from R.
 * OFDM_E_INVALID, before any launch: a null plan or hist; n_edges outside [1, OFDM_MAX_PAPR_EDGES]; an
 *   edge that is not finite, not positive or not above its predecessor; bits == NULL on a plan with more
 *   than 8 bits on a subcarrier (as ofdm_tx); a plan with an order above 256 at all (the wide map is not
 *   built into k_papr); a layout that does not fit the LDS.  n_sym = 0: an empty call.
 * It reads no channel taps and writes no ofdm_stats.
 * Kernels (k_papr): the complex128 cyclic-prefix OFDM fixed-QAM bench shapes (64-QAM at N = 1024,
 * 256-QAM at N = 4096) with Philox streams a throughput form on the flat transmitter's map and IFFT;
 * every other plan, and any plan with caller bits, the generic transmitter's.
 */
int ofdm_papr(ofdm_plan_t plan, void* stream, const uint8_t* bits, uint64_t seed,
              int64_t sym0, int64_t n_sym, const double* edges, int32_t n_edges,
              uint64_t* hist, double* sym_out, int64_t sym_keep);

/*
 * The clipped transmitter: ofdm_tx with a soft limiter on the time-domain samples (an entry point added
 * to ABI 6: nothing of the version's existing interface changes, so the number stands; ofdm_tx itself is
 * as it was).  For every OFDM symbol take the modulated samples x[0 .. N) -- the IFFT(ortho) output for
 * OFDM, the mapped points themselves for single carrier -- before the guard is attached and before the
 * channel.  With a threshold A2 = clip_a2 > 0 on |x|^2:
 *
 *     p  = re^2 + im^2                      (in the plan's precision)
 *     x' = x                   if p <= A2
 *     x' = x * sqrt(A2 / p)    otherwise    (|x'|^2 = A2: the phase kept, the envelope limited)
 *
 * Everything downstream is computed from x': the cyclic prefix (copies of limited samples) or the zero
 * guard; the FIR across symbol boundaries, the tail a chunk's regenerated predecessor hands on included;
 * and ofdm_stats (power_sum, x_power_sum, x_peak), so the PAPR they give is that of the stream sent.
 * The scale factor is not correctly rounded (a reciprocal square root with refinement, ~1 ulp in
 * complex128, ~2 ulp in complex64); the limiter is continuous and 1-Lipschitz, so the stored samples
 * stay within the transmitter's own tolerance of the definition.  A sample within rounding of the
 * threshold may fall on either side of it; both outcomes store the same sample to that tolerance.
 *
 * clip_a2: the threshold itself, a double (rounded to float on a complex64 plan); the library never sees
 *   a level in dB.  Callers derive it as A2 = 10^(clip_db / 10) P_nom, with the nominal mean power of a
 *   time sample P_nom = (1/N) sum_k mean_i |LUT_l(k)[i]|^2 in double, inactive subcarriers contributing 0,
 *   k ascending.
 * clip_counters: optional device uint64 [2], accumulated, not zeroed (NULL: nothing is counted):
 *   [0] += samples with p > A2, [1] += samples examined -- N per symbol of [sym0, sym0 + n_sym).  The
 *   guard, inactive symbols past the call's last and a chunk's regenerated predecessor are limited where
 *   they feed the stream and never counted.  Integers: identical for any batching, grid and rank count.
 * Every other argument: as ofdm_tx.
 * OFDM_E_INVALID, before any launch: what ofdm_tx refuses; clip_a2 not finite or <= 0; a plan with an
 *   order above 256 (the wide map has no limiter built in).  n_sym = 0: an empty call.
 * Kernels (k_tx, CLIP): the complex128 N = 1024 64-QAM cyclic-prefix OFDM shapes with Philox streams on
 * the flat and the 8-tap window-FIR throughput transmitters (the flat one, whose symbol leaves the IFFT
 * multiplied by h0, compares against A2 |h0|^2, the product formed on the host in double: the limiter
 * commutes with a complex scalar); every other plan, and any plan with caller bits, the generic one.
 */
int ofdm_tx_clip(ofdm_plan_t plan, void* stream, const uint8_t* bits, uint64_t seed,
                 int64_t sym0, int64_t n_sym, void* y, ofdm_stats* stats,
                 double clip_a2, uint64_t* clip_counters);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_HIP_H */
