// ofdm_launch.hpp -- POD kernel argument blocks shared by host (ofdm_abi.hip) and
// device (ofdm_kernels.hpp), plus the per-precision launcher entry points.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ofdm_device.hpp"
#include "ofdm_hip.h"
#include "ofdm_hip_soft.h"

// Diagnostic ablation switches (timing studies: tools/ablate.py, tools/power_probe.py) exist only in
// builds made with `make VARIANT=ablate EXTRA=-DOFDM_ABLATION=1`; the product library compiles
// every switch out of the kernels and never reads OFDM_ABLATE_TX / OFDM_ABLATE_RX.
#ifndef OFDM_ABLATION
#define OFDM_ABLATION 0
#endif

namespace ofdm {

__host__ __device__ constexpr int ablation_flags(int f) { return OFDM_ABLATION ? f : 0; }

constexpr int kMaxGrid = 4096;  // partial-sum workspace rows
static inline int clamp_grid(int64_t want) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, kMaxGrid));
}
// fused TX partials per workgroup: sum |y|^2 as fixed-point limbs (2 x u64), sum |x|^2, max |x|^2
constexpr int kTxFields = 4;
constexpr int kMaxTaps = 32;
constexpr int kWinTaps = 8;  // taps of the register-window FIR (LT = 4 / 8)
// LUT pool of a plan whose orders are all <= 256: the pool the fused kernels stage in LDS (the
// generic kernel in dynamic LDS, the adaptive throughput kernel in static LDS)
constexpr int kMaxLut = 512;
// largest constellation order (12 bits per subcarrier), and the pool of a plan that has an order
// above 256: such a plan's LUTs are never staged (WideAxis, ofdm_device.hpp), so the pool is bounded
// only by the plan's tables.  The reference's QAM pool 4 + 16 + ... + 4096 is 5460 entries, its
// eight largest PSK orders 32 + ... + 4096 are 8160.
constexpr int kMaxOrder = 4096;
constexpr int kMaxPool = 8192;
// bits per subcarrier the throughput (Philox) stream carries: one byte of the lane block per element
constexpr int kMaxStreamBits = 8;
// LUTs per plan: adaptive loading uses one per distinct order (PSK: 2 .. 256, eight orders)
constexpr int kMaxLuts = 8;

struct RowsArgs {
    const void* in;
    void* out;
    int64_t n_rows, in_stride, out_stride;
    int in_off, out_cp, inverse, eq;
    int zp;  // zero-padding length: modulate appends zeros, demodulate folds the tail (overlap-add)
    double scale, snr_lin, gain_mean;
    const void* tw;
    const void* eq_a;
    const void* eq_b;
};

struct EqArgs {
    const void* Y;
    void* Z;
    int64_t n_rows;
    int n, eq;
    double snr_lin, gain_mean;
    const void* eq_a;
    const void* eq_b;
};

struct MapArgs {
    const uint8_t* bytes;
    int64_t n_bytes, n_out;
    void* out;
    const void* lut;
    int b, adaptive, n_fft, bps;
    const ScInfo* sc;
    const AxisInfo* axis;
};

struct DemapArgs {
    const void* z;
    uint8_t* bytes;
    int64_t n_bytes, total_bits;
    int b, adaptive, n_fft, bps, n_active;
    const ScInfo* sc;
    const AxisInfo* axis;
    const int32_t* active;
    const double* lut64;
    const WideAxis* wide;  // per LUT, for sides above 16
};

struct DemapCountArgs {
    const void* z;            // (n_sym, N) equalised symbols
    const uint8_t* tx;        // packed tx bits, OFDM symbol s at bit s * bps
    int64_t n_sym, n_valid_bits, n_tx_bytes;
    int n_fft, b, bps, adaptive, separable;
    const ScInfo* sc;
    const AxisInfo* axis;
    const double* lut64;
    int lut_len;
    unsigned long long* counters;
    const WideAxis* wide;  // per LUT, for sides above 16
};

struct ConvArgs {
    const void* s;
    void* y;
    int64_t len;
    const void* h;
    int L;
    double* partials;
};

struct PowerArgs {
    const void* y;
    int64_t len;
    double* partials;
};

struct AwgnArgs {
    void* y;
    int64_t len;
    const double* nr;
    const double* ni;
    const double* power_sum;
    double snr_lin;
};

struct TxRxCommon {
    const uint8_t* bits;
    int64_t n_bytes;
    uint64_t seed;
    int64_t sym0, n_sym;
    const void* tw;
    const void* ptw;  // per-pass twiddle tables [forward | inverse], tt_size(logn) each
    const void* lut;
    int lut_len;
    const AxisInfo* axis;
    int n_axis;
    const ScInfo* sc;
    int adaptive, b, bps, cp, eq;
    int words_per_sym;  // LDS words staged per OFDM symbol (stream + misalignment + slack)
    double scale, gain_mean;
    const void* eq_a;
    const void* eq_b;
    // generic-kernel variants: single-carrier OFDM, zero-padding guard,
    // nearest-point decisions over the double LUT for non-separable constellations (PSK)
    int scm, zpad, nn;
    int ystride;  // stored channel samples per OFDM symbol: N, or N + cp with zero padding
    const double* lut64;
    int upat;  // every LUT has the reference's square-QAM level patterns (kUPat): adaptive fast path
    int psk_m;          // > 0: the single LUT is the reference's M-PSK (M <= 32): sector decisions
    float psk_tan[4];   // tan((q + 1/2) 2 pi / M), q < M / 8 (complex64)
    double psk_tan64[4];  // the same in double (complex128)
};

struct TxArgs {
    TxRxCommon c;
    void* y;
    double* partials;
    const void* h;
    int L;
    int chunk;
    int slot;   // complex elements per symbol row in LDS
    int flags;  // diagnostic ablation (OFDM_ABLATION builds, OFDM_ABLATE_TX): 1 no bit staging, 2 no FFT,
                // 4 no y store
    // complex128 window FIR: the first kWinTaps taps in Gauss form (re, re + im, im - re), read
    // from the kernel arguments into scalar registers (the taps are wave-uniform)
    double gtap[3][kWinTaps];
    // a plan with an order above 256 (generic kernel only): its per-LUT level tables; the kernel maps
    // through them (non-separable LUTs: from the plan's global LUT) and stages no LUT (c.lut_len = 0)
    const WideAxis* wide;
};

// ofdm_tx_clip: the limiter's arguments, a second kernel parameter behind TxArgs (k_tx CLIP
// instantiations only; every other k_tx takes TxArgs alone, as before).  a2 is the threshold on |x|^2
// the kernel compares against: the flat throughput form, whose symbol leaves the IFFT multiplied by
// h0, is handed A2 |h0|^2.
struct TxClipTail {
    double a2;
    unsigned long long* counters;  // device uint64[2] (samples clipped, samples examined), accumulated, or null
};

struct RxArgs {
    TxRxCommon c;
    const void* y;
    const double* nr;
    const double* ni;
    const double* stats;
    int64_t total_samples;
    double snr_lin;
    int noise_on;
    int64_t n_valid_bits;
    uint64_t* counters;
    void* z_out;
    int64_t z_keep;
    int flags;  // diagnostic ablation (OFDM_ABLATION builds, OFDM_ABLATE_RX): 1 no noise, 2 no FFT, 4 no bit staging,
                // 8 no equalise/demap/compare, 16 no y load
    // Host side only (the launchers read it, no kernel does; it sits in the padding behind `flags`, so the
    // kernels' argument offsets are what they were): an MMSE plan with an exact zero in its response
    // (the plan's zero_tie).  The equalised symbol of that subcarrier is an exact zero, whose decision is
    // AxisInfo::zero_i / zero_q -- a tie only the generic kernel's slicers resolve, so no launcher gives
    // such a call a throughput form (philox_streams, rx_one, rx_sweep_one).
    int zero_tie;
    const WideAxis* wide;  // a plan with an order above 256 (generic kernel only): per-LUT level patterns
    // ofdm_rx_profile: the run's per-subcarrier record, int64[5][N] (ofdm_hip.h); read by k_rx_prof only
    int64_t* profile;
};

// ofdm_rx_frames: the frame record's arguments, a second kernel parameter behind RxArgs (k_rx_frames, and
// behind RxSweepArgs k_rx_sweep_frames, whose record is uint64[n_snr][n_frames][2] and n_frames the rows
// of one point; every other receiver takes its arguments alone, as before).  The host does the 64-bit part
// of the frame index: global symbol sym0 + sl (sl: the call-relative index, < 2^31) lies in frame
//   base                              for sl < first,
//   base + 1 + (sl - first) / flen    otherwise (a 32-bit division),
// base = floor(sym0 / F), first = min(F - sym0 mod F, 2^31): the call's symbols before its first frame
// boundary, flen = min(F, 2^32 - 1) (an F beyond the call's reach has no second boundary in it).
struct RxFramesTail {
    unsigned long long* frames;  // device uint64[n_frames][2] (bit errors, symbol errors), accumulated
    int64_t base;
    int64_t n_frames;
    uint32_t first;
    uint32_t flen;
};

// ofdm_rx_density: the constellation-density record's arguments, a second kernel parameter behind RxArgs
// (k_rx_dens only; every other receiver takes its arguments alone, as before).  The grid is what the
// host made of it (ofdm_hip.h): the kernel sees lo and inv_w, never the extent.
//   flush: symbol-loop iterations a workgroup makes before it must add its 32-bit LDS bins to the
//   record and zero them -- the launcher's floor((2^32 - 1) / (points one iteration can bin)), so that no
//   bin can wrap whatever the points do
struct RxDensTail {
    unsigned long long* hist;  // device uint64[bins * bins + 1] (row = imaginary bin; last: outside), accumulated
    double lo, inv_w;
    int bins;
    int k_lo, k_hi;
    uint32_t flush;
};

// ofdm_rx_soft: the soft-decision record's arguments, a second kernel parameter behind RxArgs (k_rx_soft
// only; every other receiver takes its arguments alone, as before).  g and inv_w are what the host made
// of the weights and the extent (ofdm_hip_soft.h): the kernel sees neither.
//   lev: the plan's level table, double[n_luts][2][kSoftSide] -- per LUT the I levels LUT[a].re, then the Q
//   levels LUT[a << hb].im, by index bits a (ofdm_abi.hip, plan creation); the kernel stages it in LDS
//   flush: as RxDensTail's -- one iteration puts at most one bit of each element into one bin, so the
//   launcher's floor((2^32 - 1) / (SPB * N)) iterations cannot wrap a 32-bit bin
constexpr int kSoftSide = 16;                // levels per axis at most (256-QAM)
constexpr int kSoftRows = OFDM_SOFT_ROWS;    // 2 + 4 + 6 + 8 bits of the four orders
struct RxSoftTail {
    unsigned long long* hist;  // device uint64[kSoftRows][2][bins] + 1 (last: invalid), accumulated
    const double* g;           // device double[N]: the subcarrier's scale w_k / step_k^2
    const double* lev;
    double inv_w;
    int bins;
    int k_lo, k_hi;
    uint32_t flush;
};

// ofdm_rx_sweep: the receiver's arguments (counters: device uint64[n_snr][2]; snr_lin, noise_on,
// nr / ni, z_out, wide and profile of `r` unused: noise is always on) and the points' 10^(snr_db/10)
struct RxSweepArgs {
    RxArgs r;
    int n_snr;
    double snr_lin[OFDM_MAX_SWEEP_POINTS];
};

// ofdm_link: the receiver's arguments (y, nr / ni, z_out, wide and profile unused) and the channel's
// one tap, which the transmitter folds into its LUT; ofdm_link_screen, ofdm_link_nscreen: the screen's
// mode (OFDM_LINK_SCREEN_*; ofdm_link: automatic) and its counts.  Which screen a launch runs is
// launch_link's `screen`, not a field: the kernels' arguments stay what they were.
struct LinkArgs {
    RxArgs r;
    const void* h;
    int mode;
    // device uint64[2] (symbols screened, symbols redone), accumulated, or null; kLinkScreenSparse:
    // uint64[4], quads tested and quads sliced behind them
    unsigned long long* screen_counts;
};
// k_link's SCREEN and launch_link's `screen`: none, the two-transform float32 screen, the noise screen,
// the noise screen slicing only the quads its noise can reach (ofdm_link_inst.hpp)
constexpr int kLinkScreenNone = 0, kLinkScreenTwo = 1, kLinkScreenNoise = 2, kLinkScreenSparse = 3;

// ofdm_papr: the transmitter's common arguments (no channel, no statistics), the histogram, the optional
// per-symbol trace and the edges (linear ratios, strictly increasing)
struct PaprArgs {
    TxRxCommon c;
    unsigned long long* hist;  // device uint64[n_edges + 1], accumulated
    double* sym_out;           // device double[sym_keep][2] (peak, sum), or null
    int64_t sym_keep;
    int n_edges;
    double edges[OFDM_MAX_PAPR_EDGES];
};

// complex elements per symbol row of the fused TX: the FFT's padded row, or the extended stream if longer
constexpr int tx_slot(int logn, int cp, int L) {
    const int ext = (1 << logn) + cp + (L > 1 ? L - 1 : 0);
    return padded_row(1 << logn) > ext ? padded_row(1 << logn) : ext;
}

// The launchers' own verdicts: values of hipError_t's range that are no enumerator of it (the largest
// is 1054), so no HIP call can return one.  ofdm_abi.hip's checked() is the one place that translates
// them; nothing was launched when a launcher answers one.
//   kNotInBuild: a shape this build does not instantiate (OFDM_AB_ONLY experiment builds: N = 1024..4096
//     only) -- OFDM_E_INVALID "kernel not in this build".  Product builds instantiate every shape a plan
//     accepts and never return it.
//   kLdsOverflow: a fused launcher's shape whose LDS layout does not fit a CU (kLdsPerCu) --
//     OFDM_E_INVALID naming the shape.
//   kNoFusedForm: launch_link's plan or arguments have no fused form -- OFDM_E_INVALID.
#ifdef OFDM_AB_ONLY
constexpr bool kAbOnly = true;
#else
constexpr bool kAbOnly = false;
#endif
constexpr hipError_t kNotInBuild = static_cast<hipError_t>(2001);  // (only ever answered when kAbOnly)
constexpr hipError_t kLdsOverflow = static_cast<hipError_t>(2002);
constexpr hipError_t kNoFusedForm = static_cast<hipError_t>(2003);

// ---- launchers (instantiated for float and double in ofdm_kernels_f{32,64}.hip)
template <typename R>
hipError_t launch_rows(int logn, int mode, const RowsArgs& a, hipStream_t s);
template <typename R>
hipError_t launch_equalize(const EqArgs& a, hipStream_t s);
template <typename R>
hipError_t launch_map(const MapArgs& a, hipStream_t s);
template <typename R>
hipError_t launch_demap(const DemapArgs& a, hipStream_t s);
template <typename R>
hipError_t launch_demap_count(const DemapCountArgs& a, hipStream_t s);
template <typename R>
hipError_t launch_conv(const ConvArgs& a, int grid, hipStream_t s);
template <typename R>
hipError_t launch_power(const PowerArgs& a, int grid, hipStream_t s);
template <typename R>
hipError_t launch_awgn(const AwgnArgs& a, hipStream_t s);
// the fused launchers pick the kernel, its workgroup size and its grid; the two transmitters return
// the grid used (launch_finalize_tx reduces that many partial records)
template <typename R>
hipError_t launch_tx(int logn, const TxArgs& a, int* grid, hipStream_t s);
template <typename R>
hipError_t launch_rx(int logn, const RxArgs& a, hipStream_t s);
// the receiver with the per-subcarrier profile (a.profile set; ofdm_record_inst.hpp)
template <typename R>
hipError_t launch_rx_prof(int logn, const RxArgs& a, hipStream_t s);

// the receiver with the per-frame error record (ofdm_record_inst.hpp)
template <typename R>
hipError_t launch_rx_frames(int logn, const RxArgs& a, const RxFramesTail& f, hipStream_t s);

// the receiver with the constellation-density record (ofdm_record_inst.hpp)
template <typename R>
hipError_t launch_rx_dens(int logn, const RxArgs& a, const RxDensTail& d, hipStream_t s);

// the receiver with the soft-decision record (ofdm_record_inst.hpp); a plan with a PSK LUT or an order
// above 256 is refused by the ABI before it
template <typename R>
hipError_t launch_rx_soft(int logn, const RxArgs& a, const RxSoftTail& t, hipStream_t s);

// the one-pass SNR sweep receiver (ofdm_sweep_inst.hpp)
template <typename R>
hipError_t launch_rx_sweep(int logn, const RxSweepArgs& a, hipStream_t s);

// the sweep receiver with the per-frame error record of every point (ofdm_sweepframes_inst.hpp);
// f.frames: device uint64[a.n_snr][f.n_frames][2]
template <typename R>
hipError_t launch_rx_sweep_frames(int logn, const RxSweepArgs& a, const RxFramesTail& f, hipStream_t s);

// the fused link kernel (ofdm_link_inst.hpp; complex128 only); L: the plan's channel taps.
// kNoFusedForm: the plan or the arguments have no fused form, nothing was launched
template <typename R>
hipError_t launch_link(int logn, int L, const LinkArgs& a, int screen, hipStream_t s);

// the per-symbol PAPR histogram (ofdm_papr_inst.hpp); a plan with an order above 256 is refused by
// the ABI before it
template <typename R>
hipError_t launch_papr(int logn, const PaprArgs& a, hipStream_t s);

// the clipped transmitter (ofdm_txclip_inst.hpp); a2: A2, a2_h0: A2 |h0|^2 (the flat throughput form's
// threshold, computed on the host in double); a wide plan is refused by the ABI before it
template <typename R>
hipError_t launch_tx_clip(int logn, const TxArgs& a, double a2, double a2_h0, unsigned long long* counters, int* grid,
                          hipStream_t s);

hipError_t launch_finalize(const double* partials, int nblocks, int nfields, int max_mask,
                           double* stats, hipStream_t s);
// the fused TX's partials into an ofdm_stats record (exact fixed-point power, ofdm_hip.h)
hipError_t launch_finalize_tx(const double* partials, int nblocks, double* stats, hipStream_t s);
hipError_t launch_nn_classify(const double* lut, int m, const double* z, int64_t n, int64_t* idx,
                              hipStream_t s);
hipError_t launch_noise_radius(const uint32_t* w, int64_t n, float* r, hipStream_t s);

}  // namespace ofdm
