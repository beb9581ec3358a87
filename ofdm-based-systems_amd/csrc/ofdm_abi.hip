// ofdm_abi.hip -- C ABI of libofdm_hip.so (include/ofdm_hip.h, ofdm_hip_sweep_frames.h, ofdm_hip_soft.h): plan management,
// argument validation, error reporting, and dispatch to the gfx950 kernels.
//
// A plan owns only constant tables (twiddles, LUTs, normalised CIR, equaliser
// response) and a partial-sum workspace.  All data buffers belong to the caller.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ofdm_hip.h"
#include "ofdm_hip_soft.h"
#include "ofdm_hip_sweep_frames.h"
#include "ofdm_launch.hpp"

using namespace ofdm;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// A direct HIP API call (or a launcher that has no verdict of its own), named by its own text; the
// launchers that answer the sentinels of ofdm_launch.hpp go through checked() below
#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail(OFDM_E_HIP, std::string(#expr ": ") + hipGetErrorString(_e));      \
    } while (0)

// H[k] = sum_l h_raw[l] exp(-2 pi i (l k mod N) / N): np.fft.fft(h_raw, N)
// (simulation/models.py:264) as a direct L-tap DFT in double precision.  np.fft.fft(x, n) crops an
// input longer than n, so taps l >= N (a plan allows L = N + 1) do not enter H -- they are not
// aliased onto l mod N.
__global__ void k_taps_dft(const double* h, int L, int N, double* H) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double re = 0, im = 0;
    for (int l = 0; l < min(L, N); ++l) {
        const long long m = ((long long)l * k) % N;
        double s, c;
        sincospi(-2.0 * (double)m / (double)N, &s, &c);
        re += h[2 * l] * c - h[2 * l + 1] * s;
        im += h[2 * l] * s + h[2 * l + 1] * c;
    }
    H[2 * k] = re;
    H[2 * k + 1] = im;
}

// Equaliser tables from H (equalization/models.py:22-63):
//   ZF   : eq_a = 1 / where(H == 0, 1e-10, H)
//   MMSE : eq_a = conj(H), eq_b = |H|^2 (np.abs(H)**2)
// gsum[0] = sum |H|^2 (single block, fixed order).
template <typename R>
__global__ void k_eq_tables(const double* H, int N, int eq, R* eq_a, R* eq_b, double* gsum) {
    __shared__ double red[4];
    double acc = 0;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const double hr = H[2 * k], hi = H[2 * k + 1];
        const double a = hypot(hr, hi);
        const double g = a * a;
        acc += g;
        if (eq == OFDM_EQ_ZF) {
            double zr = hr, zi = hi;
            if (hr == 0.0 && hi == 0.0) zr = 1e-10;
            const double d = zr * zr + zi * zi;
            eq_a[2 * k] = (R)(zr / d);
            eq_a[2 * k + 1] = (R)(-zi / d);
        } else {
            eq_a[2 * k] = (R)hr;
            eq_a[2 * k + 1] = (R)(-hi);
        }
        eq_b[k] = (R)g;
    }
    acc = block_sum<double>(acc, red);
    if (threadIdx.x == 0) gsum[0] = acc;
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

struct ofdm_plan_s {
    int n, logn, cp, prec, eq, L;
    int adaptive, b, bps, n_axis, lut_len, n_active;
    double gain_mean;
    DevBuf tw, ptw, lut, lut64, h, eq_a, eq_b, axis, sc, active, H64;
    double gtap[3][kWinTaps];  // normalised taps in Gauss form (TxArgs::gtap)
    double h0_norm2;           // |h0|^2 of the first normalised tap, in double (ofdm_tx_clip: A2 |h0|^2)
    // partial-sum workspaces (3 x kMaxGrid doubles), one per HIP stream the plan has been
    // used on: launches on different streams may run concurrently, and a reduction's
    // partials must not be overwritten by another stream's kernel before k_finalize reads
    // them.  Same-stream launches are ordered, so one record per stream is enough.
    std::mutex ws_mu;
    std::map<void*, DevBuf> ws;
    int has_const, has_channel, separable, zp, single_carrier;
    int upat;  // all LUTs use the reference's square-QAM level -> index patterns (kUPat)
    int psk_m; // the single LUT is the reference's M-PSK (LUT[gray(i)] = exp(2 pi j i / M)), M <= 32
    // constellations above 256 points: max_bits = the most bits on one subcarrier; wide_plan = some
    // LUT has more than 256 entries, so the fused kernels stage no LUT and use the WideAxis table
    DevBuf wide;
    int max_bits, wide_plan;
    // ofdm_rx_soft's level table, double[n_luts][2][kSoftSide]: per LUT of side <= 16 the I levels
    // LUT[a].re and the Q levels LUT[a << hb].im by index bits a, the LUT's own doubles (zeros otherwise)
    DevBuf softlev;
    // an MMSE plan whose response is exactly zero on some subcarrier: its equalised symbol there is an
    // exact zero in every OFDM symbol, the tie AxisInfo::zero_i / zero_q decide -- every receiver
    // launch of the plan takes the generic kernel, which applies them (RxArgs::zero_tie)
    int zero_tie;
    size_t csize() const { return prec == OFDM_F32 ? 8 : 16; }
};

namespace {

template <typename T>
int upload(DevBuf& d, const T* src, size_t n, hipStream_t s) {
    if (n == 0) return OFDM_OK;
    if (hipMalloc(&d.p, n * sizeof(T)) != hipSuccess) return fail(OFDM_E_ALLOC, "hipMalloc failed");
    HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return OFDM_OK;
}

// Store complex doubles in the plan precision.
int upload_cpx(DevBuf& d, const std::vector<double>& v, int prec, hipStream_t s) {
    if (prec == OFDM_F64) return upload(d, v.data(), v.size(), s);
    std::vector<float> f(v.begin(), v.end());
    return upload(d, f.data(), f.size(), s);
}

// Decision tables for one LUT.  Square-QAM LUTs as QAMConstellationMapper.generate_constellation
// builds them (constellation/models.py:180-218) are separable: LUT[i] = lev[ki] + j lev[kq] with
// i = (qpat[kq] << b/2) | ipat[ki], which the fused slicer needs.  Any other LUT (PSK, :356-380)
// gets side = 0: map and demap gather from the LUT and search it for the nearest point, in the
// operators and in the generic fused kernels alike.
// Sides up to 16 fill AxisInfo's patterns (the throughput kernels' tables); every separable LUT,
// sides 32 and 64 included, fills its WideAxis entry: the levels, the same patterns read off the LUT,
// and their inverses for the transmitter (ofdm_device.hpp).
int build_axis(const double* lut, int m, int lut_off, AxisInfo& ax, WideAxis& wide) {
    int b = 0;
    while ((1 << b) < m) ++b;
    if (m < 2 || m > kMaxOrder || (1 << b) != m)
        return fail(OFDM_E_INVALID, "constellation order must be a power of two in [2, 4096]");
    memset(&ax, 0, sizeof(ax));
    memset(&wide, 0, sizeof(wide));
    ax.bits = b;
    ax.lut_off = lut_off;
    ax.side = 0;
    const int side = (int)std::lround(std::sqrt((double)m));
    if (side * side != m || (b & 1)) return OFDM_OK;
    std::vector<double> lev;
    for (int i = 0; i < m; ++i) lev.push_back(lut[2 * i]);
    std::sort(lev.begin(), lev.end());
    lev.erase(std::unique(lev.begin(), lev.end()), lev.end());
    if ((int)lev.size() != side) return OFDM_OK;
    const double inv_step = (side - 1) / (lev[side - 1] - lev[0]);
    std::vector<int> iset(side, -1), qset(side, -1);
    for (int i = 0; i < m; ++i) {
        const int ki = (int)(std::find(lev.begin(), lev.end(), lut[2 * i]) - lev.begin());
        const int kq = (int)(std::find(lev.begin(), lev.end(), lut[2 * i + 1]) - lev.begin());
        if (ki >= side || kq >= side) return OFDM_OK;
        const int lo = i & (side - 1), hi = i >> (b / 2);
        if ((iset[ki] >= 0 && iset[ki] != lo) || (qset[kq] >= 0 && qset[kq] != hi)) return OFDM_OK;
        iset[ki] = lo;
        qset[kq] = hi;
    }
    // uniform level spacing for the rounding slicer
    for (int k = 1; k < side; ++k)
        if (std::fabs((lev[k] - lev[k - 1]) * inv_step - 1.0) > 1e-9) return OFDM_OK;
    ax.lev0 = lev[0];
    ax.inv_step = inv_step;
    ax.side = side;
    ax.hbits = (int16_t)(b / 2);
    // A component that is exactly zero lies on the boundary between the two central levels, and the
    // origin ties between the four central points: the reference's argmin over |z - C_m| takes the
    // first index (NNClassifier, constellation/models.py:19-27).  Read that decision off the LUT: the
    // levels of the first point nearest the origin.  (The two points that share a row differ in
    // their low index bits only and the two that share a column in their high bits only, so the
    // first index of the four also decides each axis when only one component is zero.)
    int i0 = 0;
    for (int i = 1; i < m; ++i)
        if (std::hypot(lut[2 * i], lut[2 * i + 1]) < std::hypot(lut[2 * i0], lut[2 * i0 + 1])) i0 = i;
    ax.zero_i = (uint8_t)(std::find(lev.begin(), lev.end(), lut[2 * i0]) - lev.begin());
    ax.zero_q = (uint8_t)(std::find(lev.begin(), lev.end(), lut[2 * i0 + 1]) - lev.begin());
    // (every level carries exactly one index pattern per axis: m = side^2 entries over side x side
    // consistent pairs, so iset / qset are permutations of [0, side) and invert)
    static_assert(kWideSide * kWideSide == kMaxOrder, "WideAxis holds the largest side");
    for (int k = 0; k < side; ++k) {
        if (iset[k] < 0 || qset[k] < 0) return fail(OFDM_E_INVALID, "internal: incomplete level pattern");
        if (side <= 16) {
            ax.ipat[k] = (uint8_t)iset[k];
            ax.qpat[k] = (uint8_t)qset[k];
        }
        wide.lev[k] = lev[k];
        wide.ipat[k] = (uint8_t)iset[k];
        wide.qpat[k] = (uint8_t)qset[k];
        wide.inv_i[iset[k]] = (uint8_t)k;
        wide.inv_q[qset[k]] = (uint8_t)k;
    }
    // the transmitter's map must reproduce the LUT it replaces, bit for bit
    for (int i = 0; i < m; ++i)
        if (wide.lev[wide.inv_i[i & (side - 1)]] != lut[2 * i] || wide.lev[wide.inv_q[i >> (b / 2)]] != lut[2 * i + 1])
            return fail(OFDM_E_INVALID, "internal: level tables do not reproduce the LUT");
    return OFDM_OK;
}

// True when every axis maps levels to index bits like the reference's square-QAM LUTs:
// ipat[k] = U[k], qpat[k] = U[side - 1 - k] (ofdm_device.hpp, kUPat), at most 4 LUTs.
bool universal_patterns(const std::vector<AxisInfo>& axes) {
    if (axes.empty() || axes.size() > 4) return false;
    for (const AxisInfo& ax : axes) {
        if (ax.side < 2 || ax.side > 16) return false;
        for (int k = 0; k < ax.side; ++k) {
            const uint32_t u = (kUPat[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            const int kq = ax.side - 1 - k;
            const uint32_t uq = (kUPat[kq >> 2] >> (8 * (kq & 3))) & 0xFFu;
            if (ax.ipat[k] != u || ax.qpat[k] != uq) return false;
        }
    }
    return true;
}

// M if the LUT is the reference's M-PSK (constellation/models.py:356-380: LUT[gray(i)] =
// exp(2 pi j i / M)) with 2 <= M <= 32, else 0.
int psk_order(const double* lut, int m) {
    if (m < 2 || m > 32 || (m & (m - 1))) return 0;
    for (int i = 0; i < m; ++i) {
        const int g = i ^ (i >> 1);
        const double a = 2.0 * M_PI * i / m;
        if (std::fabs(lut[2 * g] - std::cos(a)) > 1e-12 || std::fabs(lut[2 * g + 1] - std::sin(a)) > 1e-12) return 0;
    }
    return m;
}

// Multipath TX: consecutive OFDM symbols per symbol group; the group's first symbol regenerates
// its predecessor's tail (one extra bits + map + IFFT per group).  32 against 16: complex128 TX
// c 5.15 -> 5.00, d 5.24 -> 5.04, e 5.19 -> 5.00 ms per step (profiles/r03ag_ab.txt).  Since each
// launch picks its chunk in [max / 2, max] to fill whole rounds of resident workgroups (tx_chunk),
// 64 (64 against 32: TX d 4.53 -> 4.44 ms, c and e within 0.5 %; 128: d 4.40, c and e 1 % slower
// and the 1e5-symbol sweep points 20 %, profiles/r05n_ab_tx_chunk.txt)
#ifndef OFDM_TX_CHUNK
#define OFDM_TX_CHUNK 64
#endif

#if OFDM_ABLATION
// Diagnostic ablation switches for timing studies (tools/ablate.py), compiled only into
// OFDM_ABLATION builds: the product library has no environment-controlled work skipping.
int env_flags(const char* name) {
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : 0;
}
#define OFDM_ENV_FLAGS(name) env_flags(name)
#else
#define OFDM_ENV_FLAGS(name) 0
#endif

int log2_exact(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return (1 << l) == n ? l : -1;
}

// 32-bit words of one OFDM symbol's bit stream staged in LDS: the stream plus a <8-bit
// misalignment of the symbol start, one slack word for the 64-bit extraction window,
// rounded up to whole Philox blocks (4 words).
int lds_words_per_sym(int bps) { return (((bps + 7 + 31) / 32 + 1) + 3) & ~3; }

// The plan's precision as a type: f(float{}) or f(double{})
template <typename F>
hipError_t with_prec(ofdm_plan_t p, F f) {
    return p->prec == OFDM_F32 ? f(float{}) : f(double{});
}

// The generic fused kernel's LDS layout for this shape exceeds a CU's (launcher: kLdsOverflow).
// (extra: what the entry point being served adds to the receiver's layout, named in the message --
// ofdm_rx_density's histogram -- and empty otherwise)
int lds_overflow(ofdm_plan_t p, const char* who, const std::string& extra) {
    return fail(OFDM_E_INVALID, std::string(who) + ": the shape" + extra + " does not fit the LDS of a compute unit (n_fft " +
                                    std::to_string(p->n) + ", " + (p->prec == OFDM_F32 ? "complex64" : "complex128") +
                                    ", prefix " + std::to_string(p->cp) + ", " + std::to_string(p->L) + " taps, " +
                                    std::to_string(p->bps) + " bits per OFDM symbol, LUT pool " +
                                    std::to_string(p->lut_len) + ")");
}

// A launcher's answer as entry point `who`'s: the one place that translates the launchers' verdicts
// (ofdm_launch.hpp; no HIP call can return one) -- bad arguments, each naming its reason; kNotInBuild is
// a dispatch that reached a shape an OFDM_AB_ONLY experiment build does not instantiate -- and reports
// any other failure as a HIP error under the entry point's name.  (layout_extra: lds_overflow's)
int checked(const char* who, ofdm_plan_t p, hipError_t e, const std::string& layout_extra = {}) {
    if (e == hipSuccess) return OFDM_OK;
    if (e == kLdsOverflow) return lds_overflow(p, who, layout_extra);
    if (e == kNoFusedForm) return fail(OFDM_E_INVALID, "ofdm_link: no fused form for this plan");
    if (kAbOnly && e == kNotInBuild)
        return fail(OFDM_E_INVALID, std::string(who) + ": kernel not in this build (an OFDM_AB_ONLY variant "
                                                       "instantiates N = 1024..4096 only)");
    return fail(OFDM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int ofdm_abi_version(void) { return OFDM_ABI_VERSION; }

const char* ofdm_last_error(void) { return g_err.c_str(); }

int ofdm_plan_create(ofdm_plan_t* out, const ofdm_desc* d, void* stream) {
    if (!out || !d) return fail(OFDM_E_INVALID, "null argument");
    *out = nullptr;
    hipStream_t s = (hipStream_t)stream;
    const int logn = log2_exact(d->n_fft);
    if (d->n_fft < 1 || d->n_fft > 4096 || logn < 0)
        return fail(OFDM_E_INVALID, "n_fft must be a power of two in [1, 4096]");
    if (d->cp < 0) return fail(OFDM_E_INVALID, "Prefix length must be a non-negative integer.");
    if (d->cp > d->n_fft) return fail(OFDM_E_INVALID, "Input symbols length must be greater than prefix length.");
    if (d->precision != OFDM_F32 && d->precision != OFDM_F64) return fail(OFDM_E_INVALID, "bad precision");
    if (d->equalizer < 0 || d->equalizer > 2) return fail(OFDM_E_INVALID, "bad equalizer");
    if (d->n_taps < 0 || d->n_taps > kMaxTaps) return fail(OFDM_E_INVALID, "n_taps must be in [0, 32]");
    if (d->n_luts < 0 || d->n_luts > kMaxLuts) return fail(OFDM_E_INVALID, "n_luts must be in [0, 8]");

    ofdm_plan_s* p = new ofdm_plan_s();
    std::unique_ptr<ofdm_plan_s> guard(p);
    p->n = d->n_fft;
    p->logn = logn;
    p->cp = d->cp;
    p->prec = d->precision;
    p->eq = d->equalizer;
    p->L = d->n_taps;
    p->gain_mean = 0;
    if (d->prefix != OFDM_PREFIX_CYCLIC && d->prefix != OFDM_PREFIX_ZERO)
        return fail(OFDM_E_INVALID, "bad prefix kind");
    p->zp = d->prefix == OFDM_PREFIX_ZERO;
    if (d->modulator != OFDM_MOD_OFDM && d->modulator != OFDM_MOD_SC) return fail(OFDM_E_INVALID, "bad modulator kind");
    p->single_carrier = d->modulator == OFDM_MOD_SC;
    if (p->zp && p->cp > p->n) return fail(OFDM_E_INVALID, "zero padding needs prefix length <= n_fft");
    p->adaptive = d->sc_lut != nullptr;
    p->has_const = d->n_luts > 0;
    p->has_channel = d->n_taps > 0 || d->H != nullptr;
    int rc;

    // twiddles lo[j] = W_N^j (j < 64), hi[j] = W_N^(64 j)
    {
        std::vector<double> tw(2 * 128, 0.0);
        const double N = (double)p->n;
        for (int j = 0; j < 64; ++j) {
            const double a = -2.0 * M_PI * (double)(j % p->n) / N;
            tw[2 * j] = std::cos(a);
            tw[2 * j + 1] = std::sin(a);
            const long long m = (64LL * j) % p->n;
            const double a2 = -2.0 * M_PI * (double)m / N;
            tw[2 * (64 + j)] = std::cos(a2);
            tw[2 * (64 + j) + 1] = std::sin(a2);
        }
        if ((rc = upload_cpx(p->tw, tw, p->prec, s))) return rc;
    }
    // per-pass twiddle tables of the throughput kernels (ofdm_device.hpp tt_from):
    // [forward | inverse], pass (LOGR, LOGNS > 0): T[(r-1) NS + k] = exp(-+2 pi i k r / (NS RAD)),
    // r = 1 only for compact passes (tt_compact)
    if (p->logn > 4) {
        const int tts = tt_size(p->logn);
        std::vector<double> tt(4 * (size_t)tts, 0.0);
        size_t at = 0;
        for (int logns = 0; logns < p->logn;) {
            const int logr = std::min(4, p->logn - logns);
            const int ns = 1 << logns, rad = 1 << logr;
            if (logns > 0) {
                const int rmax = tt_compact(p->logn, logns) ? 2 : rad;  // compact: W^k only
                for (int r = 1; r < rmax; ++r)
                    for (int k = 0; k < ns; ++k, ++at) {
                        const double a = -2.0 * M_PI * (double)(k * r) / (double)(ns * rad);
                        tt[2 * at] = std::cos(a);
                        tt[2 * at + 1] = std::sin(a);
                        tt[2 * (tts + at)] = std::cos(a);
                        tt[2 * (tts + at) + 1] = -std::sin(a);
                    }
            }
            logns += logr;
        }
        if ((int)at != tts) return fail(OFDM_E_INVALID, "internal: twiddle table size");
        if ((rc = upload_cpx(p->ptw, tt, p->prec, s))) return rc;
    }

    // constellations
    if (p->has_const) {
        std::vector<AxisInfo> axes(d->n_luts);
        std::vector<WideAxis> wides(d->n_luts);
        int off = 0, top = 0;
        for (int i = 0; i < d->n_luts; ++i) {
            // (the order is checked before the LUT is read: off stays within the caller's pool)
            if ((rc = build_axis(d->lut_pool + 2 * off, d->lut_orders[i], off, axes[i], wides[i]))) return rc;
            off += d->lut_orders[i];
            top = std::max(top, (int)d->lut_orders[i]);
        }
        // orders up to 256: the pool the fused kernels stage in LDS; above: never staged
        p->wide_plan = top > 256;
        if (off > (p->wide_plan ? kMaxPool : kMaxLut))
            return fail(OFDM_E_INVALID, p->wide_plan ? "LUT pool too large (more than 8192 entries)"
                                                     : "LUT pool too large (more than 512 entries with every order <= 256)");
        p->lut_len = off;
        p->n_axis = d->n_luts;
        p->separable = 1;
        for (const AxisInfo& ax : axes) p->separable &= ax.side > 0;
        p->upat = p->separable && universal_patterns(axes);
        p->psk_m = (!p->separable && d->n_luts == 1) ? psk_order(d->lut_pool, d->lut_orders[0]) : 0;
        std::vector<double> pool(d->lut_pool, d->lut_pool + 2 * off);
        if ((rc = upload_cpx(p->lut, pool, p->prec, s))) return rc;
        if ((rc = upload(p->lut64, pool.data(), pool.size(), s))) return rc;
        if ((rc = upload(p->axis, axes.data(), axes.size(), s))) return rc;
        if ((rc = upload(p->wide, wides.data(), wides.size(), s))) return rc;
        {
            std::vector<double> sl((size_t)d->n_luts * 2 * kSoftSide, 0.0);
            for (int i = 0; i < d->n_luts; ++i) {
                const AxisInfo& ax = axes[i];
                if (ax.side < 2 || ax.side > kSoftSide) continue;
                for (int a = 0; a < ax.side; ++a) {
                    sl[((size_t)i * 2 + 0) * kSoftSide + a] = d->lut_pool[2 * (ax.lut_off + a)];
                    sl[((size_t)i * 2 + 1) * kSoftSide + a] = d->lut_pool[2 * (ax.lut_off + (a << ax.hbits)) + 1];
                }
            }
            if ((rc = upload(p->softlev, sl.data(), sl.size(), s))) return rc;
        }
        p->max_bits = 0;
        if (p->adaptive) {
            std::vector<ScInfo> sc(p->n);
            std::vector<int32_t> act;
            int bit = 0;
            for (int k = 0; k < p->n; ++k) {
                const int id = d->sc_lut[k];
                if (id < -1 || id >= d->n_luts) return fail(OFDM_E_INVALID, "sc_lut entry out of range");
                sc[k].lut = (int16_t)id;
                sc[k].bits = (int16_t)(id < 0 ? 0 : axes[id].bits);
                sc[k].bitoff = bit;
                bit += sc[k].bits;
                p->max_bits = std::max(p->max_bits, (int)sc[k].bits);
                if (id >= 0) act.push_back(k);
            }
            if (bit == 0) return fail(OFDM_E_INVALID, "No active subcarriers (all orders are zero)");
            p->bps = bit;
            p->b = -1;
            p->n_active = (int)act.size();
            if ((rc = upload(p->sc, sc.data(), sc.size(), s))) return rc;
            if ((rc = upload(p->active, act.data(), act.size(), s))) return rc;
        } else {
            if (d->n_luts != 1) return fail(OFDM_E_INVALID, "fixed mode takes exactly one LUT");
            p->b = axes[0].bits;
            p->max_bits = p->b;
            p->bps = p->b * p->n;
            p->n_active = p->n;
        }
    } else {
        p->lut_len = 0;
        p->n_axis = 0;
        p->separable = 0;
        p->b = 0;
        p->bps = 0;
        p->n_active = 0;
    }

    // channel: normalised taps for the convolution, H for the equaliser
    if (d->n_taps > 0) {
        double pw = 0;
        for (int l = 0; l < d->n_taps; ++l)
            pw += d->h_raw[2 * l] * d->h_raw[2 * l] + d->h_raw[2 * l + 1] * d->h_raw[2 * l + 1];
        if (pw == 0) return fail(OFDM_E_INVALID, "Impulse response cannot be all zeros.");
        const double sc = std::sqrt(pw);
        std::vector<double> hn(2 * d->n_taps);
        for (int l = 0; l < 2 * d->n_taps; ++l) hn[l] = d->h_raw[l] / sc;
        if ((rc = upload_cpx(p->h, hn, p->prec, s))) return rc;
        p->h0_norm2 = hn[0] * hn[0] + hn[1] * hn[1];
        for (int l = 0; l < kWinTaps; ++l) {
            const double re = l < d->n_taps ? hn[2 * l] : 0.0, im = l < d->n_taps ? hn[2 * l + 1] : 0.0;
            p->gtap[0][l] = re;
            p->gtap[1][l] = re + im;
            p->gtap[2][l] = im - re;
        }
    }
    if (p->has_channel) {
        if (hipMalloc(&p->H64.p, 16 * (size_t)p->n) != hipSuccess) return fail(OFDM_E_ALLOC, "hipMalloc failed");
        if (d->H) {
            HIPCHK(hipMemcpyAsync(p->H64.p, d->H, 16 * (size_t)p->n, hipMemcpyHostToDevice, s));
        } else {
            DevBuf hr;
            std::vector<double> hv(d->h_raw, d->h_raw + 2 * d->n_taps);
            if ((rc = upload(hr, hv.data(), hv.size(), s))) return rc;
            (void)hipGetLastError();
            hipLaunchKernelGGL(k_taps_dft, dim3((p->n + 255) / 256), dim3(256), 0, s, (const double*)hr.p,
                               d->n_taps, p->n, (double*)p->H64.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));
        }
        if (hipMalloc(&p->eq_a.p, p->csize() * p->n) != hipSuccess ||
            hipMalloc(&p->eq_b.p, p->csize() / 2 * p->n) != hipSuccess)
            return fail(OFDM_E_ALLOC, "hipMalloc failed");
        DevBuf g;
        if (hipMalloc(&g.p, sizeof(double)) != hipSuccess) return fail(OFDM_E_ALLOC, "hipMalloc failed");
        const int eqk = p->eq == OFDM_EQ_ZF ? OFDM_EQ_ZF : OFDM_EQ_MMSE;
        if (p->prec == OFDM_F32)
            hipLaunchKernelGGL(k_eq_tables<float>, dim3(1), dim3(256), 0, s, (const double*)p->H64.p, p->n, eqk,
                               (float*)p->eq_a.p, (float*)p->eq_b.p, (double*)g.p);
        else
            hipLaunchKernelGGL(k_eq_tables<double>, dim3(1), dim3(256), 0, s, (const double*)p->H64.p, p->n, eqk,
                               (double*)p->eq_a.p, (double*)p->eq_b.p, (double*)g.p);
        HIPCHK(hipGetLastError());
        double gs = 0;
        HIPCHK(hipMemcpyAsync(&gs, g.p, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        p->gain_mean = gs / p->n;
        if (p->eq == OFDM_EQ_MMSE) {
            std::vector<double> Hh(2 * (size_t)p->n);
            HIPCHK(hipMemcpyAsync(Hh.data(), p->H64.p, 16 * (size_t)p->n, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (int k = 0; k < p->n; ++k)
                if (Hh[2 * k] == 0.0 && Hh[2 * k + 1] == 0.0) p->zero_tie = 1;
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    *out = guard.release();
    return OFDM_OK;
}

int ofdm_plan_destroy(ofdm_plan_t plan) {
    delete plan;
    return OFDM_OK;
}

int ofdm_plan_get_info(ofdm_plan_t p, ofdm_plan_info* info) {
    if (!p || !info) return fail(OFDM_E_INVALID, "null argument");
    info->n_fft = p->n;
    info->cp = p->cp;
    info->precision = p->prec;
    info->equalizer = p->eq;
    info->n_taps = p->L;
    info->bits_per_ofdm_symbol = p->bps;
    info->bits_per_subcarrier = p->adaptive ? -1 : p->b;
    info->adaptive = p->adaptive;
    info->channel_gain_mean = p->gain_mean;
    return OFDM_OK;
}

int ofdm_plan_response(ofdm_plan_t p, void* stream, double* H, double* gains) {
    if (!p || !H) return fail(OFDM_E_INVALID, "null argument");
    if (!p->has_channel) return fail(OFDM_E_INVALID, "plan has no channel response");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(H, p->H64.p, 16 * (size_t)p->n, hipMemcpyDeviceToDevice, s));
    if (gains) {
        if (p->prec == OFDM_F64) {
            HIPCHK(hipMemcpyAsync(gains, p->eq_b.p, 8 * (size_t)p->n, hipMemcpyDeviceToDevice, s));
        } else {
            return fail(OFDM_E_INVALID, "gains are exported by float64 plans only");
        }
    }
    return OFDM_OK;
}

int ofdm_fft(ofdm_plan_t p, void* stream, void* data, int64_t batch, int32_t inverse) {
    if (!p || (!data && batch > 0) || batch < 0) return fail(OFDM_E_INVALID, "bad argument to ofdm_fft");
    RowsArgs a{};
    a.in = data;
    a.out = data;
    a.n_rows = batch;
    a.in_stride = p->n;
    a.out_stride = p->n;
    a.inverse = inverse != 0;
    a.scale = 1.0 / std::sqrt((double)p->n);
    a.tw = p->tw.p;
    return checked("ofdm_fft", p, with_prec(p, [&](auto r) {
        return launch_rows<decltype(r)>(p->logn, 0, a, (hipStream_t)stream);
    }));
}

int ofdm_modulate(ofdm_plan_t p, void* stream, const void* X, int64_t n_sym, void* x) {
    if (!p || n_sym < 0 || (n_sym > 0 && (!X || !x))) return fail(OFDM_E_INVALID, "bad argument to ofdm_modulate");
    RowsArgs a{};
    a.in = X;
    a.out = x;
    a.n_rows = n_sym;
    a.in_stride = p->n;
    a.out_stride = p->n + p->cp;
    a.out_cp = p->cp;
    a.zp = p->zp ? p->cp : 0;
    a.scale = 1.0 / std::sqrt((double)p->n);
    a.tw = p->tw.p;
    return checked("ofdm_modulate", p, with_prec(p, [&](auto r) {
        return launch_rows<decltype(r)>(p->logn, 1, a, (hipStream_t)stream);
    }));
}

int ofdm_demodulate(ofdm_plan_t p, void* stream, const void* yt, int64_t n_sym, double snr_db, void* Z) {
    if (!p || n_sym < 0 || (n_sym > 0 && (!yt || !Z))) return fail(OFDM_E_INVALID, "bad argument to ofdm_demodulate");
    if (p->eq != OFDM_EQ_NONE && !p->has_channel) return fail(OFDM_E_INVALID, "plan has no channel response");
    RowsArgs a{};
    a.in = yt;
    a.out = Z;
    a.n_rows = n_sym;
    a.in_stride = p->n + p->cp;
    a.in_off = p->zp ? 0 : p->cp;
    a.zp = p->zp ? p->cp : 0;
    a.out_stride = p->n;
    a.eq = p->eq;
    a.scale = 1.0 / std::sqrt((double)p->n);
    a.snr_lin = std::pow(10.0, snr_db / 10.0);
    a.gain_mean = p->gain_mean;
    a.tw = p->tw.p;
    a.eq_a = p->eq_a.p;
    a.eq_b = p->eq_b.p;
    return checked("ofdm_demodulate", p, with_prec(p, [&](auto r) {
        return launch_rows<decltype(r)>(p->logn, 2, a, (hipStream_t)stream);
    }));
}

int ofdm_equalize(ofdm_plan_t p, void* stream, const void* Y, int64_t n_rows, double snr_db, void* Z) {
    if (!p || n_rows < 0 || (n_rows > 0 && (!Y || !Z))) return fail(OFDM_E_INVALID, "bad argument to ofdm_equalize");
    if (p->eq != OFDM_EQ_NONE && !p->has_channel) return fail(OFDM_E_INVALID, "plan has no channel response");
    EqArgs a{};
    a.Y = Y;
    a.Z = Z;
    a.n_rows = n_rows;
    a.n = p->n;
    a.eq = p->eq;
    a.snr_lin = std::pow(10.0, snr_db / 10.0);
    a.gain_mean = p->gain_mean;
    a.eq_a = p->eq_a.p;
    a.eq_b = p->eq_b.p;
    return checked("ofdm_equalize", p, with_prec(p, [&](auto r) {
        return launch_equalize<decltype(r)>(a, (hipStream_t)stream);
    }));
}

int ofdm_map(ofdm_plan_t p, void* stream, const uint8_t* bytes, int64_t n_bytes, int64_t n_out, void* symbols) {
    if (!p || !p->has_const) return fail(OFDM_E_INVALID, "plan has no constellation");
    if (n_bytes < 0 || n_out < 0 || (n_out > 0 && !symbols) || (n_bytes > 0 && !bytes))
        return fail(OFDM_E_INVALID, "bad argument to ofdm_map");
    if (p->adaptive && n_out % p->n) return fail(OFDM_E_INVALID, "adaptive map needs whole OFDM symbols");
    MapArgs a{};
    a.bytes = bytes;
    a.n_bytes = n_bytes;
    a.n_out = n_out;
    a.out = symbols;
    a.lut = p->lut.p;
    a.b = p->b;
    a.adaptive = p->adaptive;
    a.n_fft = p->n;
    a.bps = p->bps;
    a.sc = (const ScInfo*)p->sc.p;
    a.axis = (const AxisInfo*)p->axis.p;
    return checked("ofdm_map", p, with_prec(p, [&](auto r) {
        return launch_map<decltype(r)>(a, (hipStream_t)stream);
    }));
}

int ofdm_demap(ofdm_plan_t p, void* stream, const void* z, int64_t n, uint8_t* bytes) {
    if (!p || !p->has_const) return fail(OFDM_E_INVALID, "plan has no constellation");
    if (n < 0 || (n > 0 && (!z || !bytes))) return fail(OFDM_E_INVALID, "bad argument to ofdm_demap");
    DemapArgs a{};
    a.z = z;
    a.bytes = bytes;
    if (p->adaptive) {
        if (n % p->n) return fail(OFDM_E_INVALID, "adaptive demap needs whole OFDM symbols");
        a.total_bits = (n / p->n) * (int64_t)p->bps;
        a.n_bytes = a.total_bits / 8;
    } else {
        a.total_bits = n * (int64_t)p->b;
        a.n_bytes = (a.total_bits + 7) / 8;
    }
    a.b = p->b;
    a.adaptive = p->adaptive;
    a.n_fft = p->n;
    a.bps = p->bps;
    a.n_active = p->n_active;
    a.sc = (const ScInfo*)p->sc.p;
    a.axis = (const AxisInfo*)p->axis.p;
    a.active = (const int32_t*)p->active.p;
    a.lut64 = (const double*)p->lut64.p;
    a.wide = (const WideAxis*)p->wide.p;
    return checked("ofdm_demap", p, with_prec(p, [&](auto r) {
        return launch_demap<decltype(r)>(a, (hipStream_t)stream);
    }));
}

int ofdm_demap_count(ofdm_plan_t p, void* stream, const void* Z, const uint8_t* tx_bits, int64_t n_sym,
                     uint64_t* counters) {
    if (!p || !p->has_const) return fail(OFDM_E_INVALID, "plan has no constellation");
    if (n_sym < 0 || (n_sym > 0 && (!Z || !tx_bits || !counters)))
        return fail(OFDM_E_INVALID, "bad argument to ofdm_demap_count");
    DemapCountArgs a{};
    a.z = Z;
    a.tx = tx_bits;
    a.n_sym = n_sym;
    const int64_t total = n_sym * (int64_t)p->bps;
    // the reference compares every bit in FIXED mode, whole bytes in adaptive mode (its decode
    // drops a trailing partial byte, constellation/adaptive.py:259-263)
    a.n_valid_bits = p->adaptive ? (total / 8) * 8 : total;
    a.n_tx_bytes = (total + 7) / 8;
    a.n_fft = p->n;
    a.b = p->b;
    a.bps = p->bps;
    a.adaptive = p->adaptive;
    a.separable = p->separable;
    a.sc = (const ScInfo*)p->sc.p;
    a.axis = (const AxisInfo*)p->axis.p;
    a.lut64 = (const double*)p->lut64.p;
    a.lut_len = p->lut_len;
    a.counters = (unsigned long long*)counters;
    a.wide = (const WideAxis*)p->wide.p;
    return checked("ofdm_demap_count", p, with_prec(p, [&](auto r) {
        return launch_demap_count<decltype(r)>(a, (hipStream_t)stream);
    }));
}

int ofdm_nn_classify(void* stream, const double* lut, int32_t m, const void* z, int64_t n, int64_t* idx) {
    if (m < 1 || n < 0 || !lut || (n > 0 && (!z || !idx))) return fail(OFDM_E_INVALID, "bad argument to ofdm_nn_classify");
    HIPCHK(launch_nn_classify(lut, m, (const double*)z, n, idx, (hipStream_t)stream));
    return OFDM_OK;
}

int ofdm_noise_radius(void* stream, const uint32_t* words, int64_t n, float* radius) {
    if (n < 0 || (n > 0 && (!words || !radius))) return fail(OFDM_E_INVALID, "bad argument to ofdm_noise_radius");
    HIPCHK(launch_noise_radius(words, n, radius, (hipStream_t)stream));
    return OFDM_OK;
}

// The stream's partial-sum workspace (allocated on first use), or nullptr.
static double* workspace(ofdm_plan_t p, void* stream) {
    std::lock_guard<std::mutex> lk(p->ws_mu);
    DevBuf& d = p->ws[stream];
    if (!d.p && hipMalloc(&d.p, sizeof(double) * kTxFields * kMaxGrid) != hipSuccess) {
        d.p = nullptr;
        return nullptr;
    }
    return (double*)d.p;
}

int ofdm_channel(ofdm_plan_t p, void* stream, const void* sig, int64_t len, void* y, double* power_sum) {
    if (!p || p->L < 1) return fail(OFDM_E_INVALID, "plan has no channel taps");
    if (len < 0 || (len > 0 && (!sig || !y))) return fail(OFDM_E_INVALID, "bad argument to ofdm_channel");
    if (len == 0) return OFDM_OK;
    const int grid = clamp_grid((len + 255) / 256);
    double* ws = workspace(p, stream);
    if (!ws) return fail(OFDM_E_ALLOC, "hipMalloc failed");
    ConvArgs a{sig, y, len, p->h.p, p->L, ws};
    if (int rc = checked("ofdm_channel", p, with_prec(p, [&](auto r) {
            return launch_conv<decltype(r)>(a, grid, (hipStream_t)stream);
        })))
        return rc;
    if (power_sum) HIPCHK(launch_finalize(ws, grid, 1, 0, power_sum, (hipStream_t)stream));
    return OFDM_OK;
}

int ofdm_power(ofdm_plan_t p, void* stream, const void* y, int64_t len, double* power_sum) {
    if (!p || len < 0 || (len > 0 && !y) || !power_sum) return fail(OFDM_E_INVALID, "bad argument to ofdm_power");
    if (len == 0) return OFDM_OK;
    const int grid = clamp_grid((len + 255) / 256);
    double* ws = workspace(p, stream);
    if (!ws) return fail(OFDM_E_ALLOC, "hipMalloc failed");
    PowerArgs a{y, len, ws};
    if (int rc = checked("ofdm_power", p, with_prec(p, [&](auto r) {
            return launch_power<decltype(r)>(a, grid, (hipStream_t)stream);
        })))
        return rc;
    HIPCHK(launch_finalize(ws, grid, 1, 0, power_sum, (hipStream_t)stream));
    return OFDM_OK;
}

int ofdm_awgn(ofdm_plan_t p, void* stream, void* y, int64_t len, const double* nr, const double* ni,
              const double* power_sum, double snr_db) {
    if (!p || len < 0 || (len > 0 && (!y || !nr || !ni || !power_sum)))
        return fail(OFDM_E_INVALID, "bad argument to ofdm_awgn");
    AwgnArgs a{y, len, nr, ni, power_sum, std::pow(10.0, snr_db / 10.0)};
    return checked("ofdm_awgn", p, with_prec(p, [&](auto r) {
        return launch_awgn<decltype(r)>(a, (hipStream_t)stream);
    }));
}

// Throughput mode (bits == NULL: Philox stream version 3) gives each element one byte of its lane
// block, so it carries at most kMaxStreamBits bits per subcarrier; a wider order would share bits
// between neighbouring elements.  Such a plan runs with the caller's bits only.
static int stream_bits_ok(ofdm_plan_t p, const uint8_t* bits, const char* who) {
    if (bits != nullptr || p->max_bits <= kMaxStreamBits) return OFDM_OK;
    return fail(OFDM_E_INVALID, std::string(who) + ": the throughput (Philox) bit stream carries at most 8 bits per "
                                    "subcarrier and this plan has up to " + std::to_string(p->max_bits) +
                                    "; pass the tx bits (reference-stream mode)");
}

// The supported symbol range (OFDM_MAX_SYMBOLS, ofdm_hip.h): asked after sym0 >= 0 and n_sym >= 0 are
// known, and formed as a difference, so that nothing wraps for any pair of int64_t values.
static int symbols_ok(const char* who, int64_t sym0, int64_t n_sym) {
    if (sym0 <= OFDM_MAX_SYMBOLS && n_sym <= OFDM_MAX_SYMBOLS - sym0) return OFDM_OK;
    return fail(OFDM_E_INVALID, std::string(who) + ": symbols [" + std::to_string(sym0) + ", " + std::to_string(sym0) +
                                    " + " + std::to_string(n_sym) + ") reach beyond OFDM_MAX_SYMBOLS = 2^46, the "
                                    "supported symbol range");
}

static void fill_common(ofdm_plan_t p, TxRxCommon& c, const uint8_t* bits, uint64_t seed, int64_t sym0,
                        int64_t n_sym, int64_t total_syms_for_bits) {
    c.bits = bits;
    c.n_bytes = (total_syms_for_bits * (int64_t)p->bps + 7) / 8;
    c.seed = seed;
    c.sym0 = sym0;
    c.n_sym = n_sym;
    c.tw = p->tw.p;
    c.ptw = p->ptw.p;
    c.lut = p->lut.p;
    c.lut_len = p->lut_len;
    c.axis = (const AxisInfo*)p->axis.p;
    c.n_axis = p->n_axis;
    c.sc = (const ScInfo*)p->sc.p;
    c.adaptive = p->adaptive;
    c.b = p->b;
    c.bps = p->bps;
    c.cp = p->cp;
    c.eq = p->eq;
    c.words_per_sym = lds_words_per_sym(p->bps);
    c.scale = 1.0 / std::sqrt((double)p->n);
    c.gain_mean = p->gain_mean;
    c.eq_a = p->eq_a.p;
    c.eq_b = p->eq_b.p;
    c.scm = p->single_carrier;
    c.zpad = p->zp && p->cp > 0;
    c.nn = !p->separable;
    c.ystride = c.zpad ? p->n + p->cp : p->n;
    c.lut64 = (const double*)p->lut64.p;
    c.upat = p->upat;
    // sector decisions for the reference's M-PSK in throughput mode (device bits) on the throughput
    // kernels; the reference-stream mode and the generic kernel keep the reference's nearest-point
    // search (complex128: the same decisions except on a sector boundary, ~1e-16 relative)
    c.psk_m = bits == nullptr ? p->psk_m : 0;
    for (int q = 0; q < 4; ++q) {
        const double tq = (c.psk_m >= 8 && q < c.psk_m / 8) ? std::tan((q + 0.5) * 2.0 * M_PI / c.psk_m) : 0.0;
        c.psk_tan[q] = (float)tq;
        c.psk_tan64[q] = tq;
    }
}

// ofdm_tx and ofdm_tx_clip (who; clip: the limiter's threshold and record, or null for ofdm_tx, whose
// checks, arguments and launch are then what they were)
struct TxClip {
    double a2;
    uint64_t* counters;
};
static int tx_call(const char* who, ofdm_plan_t p, void* stream, const uint8_t* bits, uint64_t seed, int64_t sym0,
                   int64_t n_sym, void* y, ofdm_stats* stats, const TxClip* clip) {
    if (!p || !p->has_const || p->L < 1)
        return fail(OFDM_E_INVALID, std::string(who) + " needs a constellation and channel taps");
    if (p->L - 1 > p->n) return fail(OFDM_E_INVALID, "fused path needs channel order <= n_fft");
    if (n_sym < 0 || sym0 < 0 || !stats) return fail(OFDM_E_INVALID, std::string("bad argument to ") + who);
    if (int rc = symbols_ok(who, sym0, n_sym)) return rc;
    if (clip) {
        if (!std::isfinite(clip->a2) || !(clip->a2 > 0.0))
            return fail(OFDM_E_INVALID, "ofdm_tx_clip: clip_a2 is not a finite positive threshold on |x|^2");
        if (p->prec == OFDM_F32 && !((float)clip->a2 > 0.f && std::isfinite((float)clip->a2)))
            return fail(OFDM_E_INVALID, "ofdm_tx_clip: clip_a2 is not a finite positive float on a complex64 plan");
    }
    if (int rc = stream_bits_ok(p, bits, who)) return rc;
    // (after stream_bits_ok: without caller bits a wide plan answers as ofdm_tx does)
    if (clip && p->wide_plan)
        return fail(OFDM_E_INVALID, "ofdm_tx_clip: the plan has a constellation above 256 points, and the wide map "
                                    "has no limiter built in (orders up to 256 only)");
    if (n_sym == 0) return OFDM_OK;
    TxArgs a{};
    // the bits buffer covers global symbols [0, sym0 + n_sym)
    fill_common(p, a.c, bits, seed, sym0, n_sym, sym0 + n_sym);
    if (p->wide_plan) {
        // an order above 256: the kernel maps from the level tables and stages no LUT
        a.wide = (const WideAxis*)p->wide.p;
        a.c.lut_len = 0;
    }
    a.y = y;
    a.partials = workspace(p, stream);
    if (!a.partials) return fail(OFDM_E_ALLOC, "hipMalloc failed");
    a.h = p->h.p;
    a.L = p->L;
    std::memcpy(a.gtap, p->gtap, sizeof a.gtap);
    a.chunk = p->L > 1 ? OFDM_TX_CHUNK : 1;
    a.slot = tx_slot(p->logn, p->cp, p->L);
    a.flags = OFDM_ENV_FLAGS("OFDM_ABLATE_TX");
    int grid = 0;  // chosen by the launcher with the kernel (<= kMaxGrid partial records)
    if (int rc = checked(who, p, with_prec(p, [&](auto r) {
            using R = decltype(r);
            return clip ? launch_tx_clip<R>(p->logn, a, clip->a2, clip->a2 * p->h0_norm2,
                                            (unsigned long long*)clip->counters, &grid, (hipStream_t)stream)
                        : launch_tx<R>(p->logn, a, &grid, (hipStream_t)stream);
        })))
        return rc;
    HIPCHK(launch_finalize_tx(a.partials, grid, (double*)stats, (hipStream_t)stream));
    return OFDM_OK;
}

int ofdm_tx(ofdm_plan_t p, void* stream, const uint8_t* bits, uint64_t seed, int64_t sym0, int64_t n_sym,
            void* y, ofdm_stats* stats) {
    return tx_call("ofdm_tx", p, stream, bits, seed, sym0, n_sym, y, stats, nullptr);
}

int ofdm_tx_clip(ofdm_plan_t p, void* stream, const uint8_t* bits, uint64_t seed, int64_t sym0, int64_t n_sym,
                 void* y, ofdm_stats* stats, double clip_a2, uint64_t* clip_counters) {
    const TxClip clip{clip_a2, clip_counters};
    return tx_call("ofdm_tx_clip", p, stream, bits, seed, sym0, n_sym, y, stats, &clip);
}

// The argument path of every fused receiver entry point (who): the plan and the common arguments checked
// in the order callers rely on -- own(): the entry point's own checks, in their place in it -- and the
// receiver's common arguments filled.  *run: false with OFDM_OK for an empty run (its stream has no
// samples and no noise power).
static int rx_args(const char* who, ofdm_plan_t p, const void* y, const double* nr, const double* ni, uint64_t seed,
                   const ofdm_stats* stats, int64_t total_samples, int32_t noise_on, const uint8_t* bits,
                   int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters,
                   const std::function<int()>& own, RxArgs& a, bool* run) {
    const std::string bad = std::string("bad argument to ") + who;
    *run = false;
    if (!p || !p->has_const) return fail(OFDM_E_INVALID, std::string(who) + " needs a constellation");
    if (p->eq != OFDM_EQ_NONE && !p->has_channel) return fail(OFDM_E_INVALID, "plan has no channel response");
    if (n_sym < 0 || sym0 < 0 || !counters) return fail(OFDM_E_INVALID, bad);
    if (int rc = symbols_ok(who, sym0, n_sym)) return rc;
    if (int rc = own()) return rc;
    if (int rc = stream_bits_ok(p, bits, who)) return rc;
    if (n_sym == 0) return OFDM_OK;
    if (!y || (noise_on && (!stats || total_samples <= 0))) return fail(OFDM_E_INVALID, bad);
    if ((nr == nullptr) != (ni == nullptr)) return fail(OFDM_E_INVALID, "nr and ni must both be given or both NULL");
    fill_common(p, a.c, bits, seed, sym0, n_sym, sym0 + n_sym);
    a.y = y;
    a.nr = nr;
    a.ni = ni;
    a.stats = (const double*)stats;
    a.total_samples = total_samples;
    a.noise_on = noise_on;
    a.n_valid_bits = n_valid_bits;
    a.counters = counters;
    a.zero_tie = p->zero_tie;
    *run = true;
    return OFDM_OK;
}

// ofdm_rx_frames' record (ofdm_hip.h)
struct RxFrames {
    int64_t frame_len, n_frames;
    uint64_t* frames;
};
// The frame record's own refusals, made before the plan is looked at (a negative sym0 or n_sym is left
// to rx_args)
static int frames_ok(const char* who, const RxFrames& fr, int64_t sym0, int64_t n_sym) {
    const auto no = [&](const std::string& why) { return fail(OFDM_E_INVALID, std::string(who) + ": " + why); };
    if (!fr.frames) return no("needs a frame record");
    if (fr.frame_len < 1) return no("frame_len " + std::to_string(fr.frame_len) + " is not a positive symbol count");
    if (fr.n_frames < 1) return no("n_frames " + std::to_string(fr.n_frames) + " is not a positive frame count");
    if (n_sym > (int64_t)1 << 31) return no("a call takes at most 2^31 symbols, got " + std::to_string(n_sym));
    if (sym0 >= 0 && n_sym > 0) {
        // the last symbol sym0 + n_sym - 1 and its frame in unsigned arithmetic: sym0 < 2^63 and
        // n_sym <= 2^31 here, so neither the sum nor floor(sym0 / F) + the carry of the remainder wraps
        const uint64_t F = (uint64_t)fr.frame_len;
        const uint64_t last = (uint64_t)sym0 + (uint64_t)(n_sym - 1);
        const uint64_t frame = (uint64_t)sym0 / F + ((uint64_t)sym0 % F + (uint64_t)(n_sym - 1)) / F;
        if (frame >= (uint64_t)fr.n_frames)
            return no("the call's last symbol " + std::to_string(last) + " lies in frame " + std::to_string(frame) +
                      ", beyond the record's " + std::to_string(fr.n_frames) + " frames");
    }
    return (int)OFDM_OK;
}
// the 64-bit part of the frame index, done on the host once (RxFramesTail)
static RxFramesTail frames_tail(const RxFrames& fr, int64_t sym0) {
    RxFramesTail ft{};
    ft.frames = (unsigned long long*)fr.frames;
    ft.base = sym0 / fr.frame_len;
    ft.n_frames = fr.n_frames;
    ft.first = (uint32_t)std::min<int64_t>(fr.frame_len - sym0 % fr.frame_len, (int64_t)1 << 31);
    ft.flen = (uint32_t)std::min<int64_t>(fr.frame_len, 0xFFFFFFFFll);
    return ft;
}
// ofdm_rx_density's record and grid (ofdm_hip.h)
struct RxDens {
    double lo, inv_w;
    int32_t bins, k_lo, k_hi;
    uint64_t* hist;
};
// The density record's own refusals, made before anything else is looked at (n_fft: the plan's, or 0
// without a plan, which rx_args then refuses)
static int dens_ok(const char* who, const RxDens& d, int n_fft) {
    const auto no = [&](const std::string& why) { return fail(OFDM_E_INVALID, std::string(who) + ": " + why); };
    if (!d.hist) return no("needs a density record");
    if (d.bins < 1 || d.bins > OFDM_MAX_DENSITY_BINS)
        return no("bins " + std::to_string(d.bins) + " is not in [1, " + std::to_string(OFDM_MAX_DENSITY_BINS) + "]");
    if (!std::isfinite(d.lo)) return no("lo is not finite");
    if (!std::isfinite(d.inv_w) || !(d.inv_w > 0)) return no("inv_w is not a finite positive bin rate");
    if (d.k_lo < 0 || d.k_lo >= d.k_hi || (n_fft > 0 && d.k_hi > n_fft))
        return no("the subcarrier range [" + std::to_string(d.k_lo) + ", " + std::to_string(d.k_hi) +
                  ") is not 0 <= k_lo < k_hi <= n_fft" + (n_fft > 0 ? " = " + std::to_string(n_fft) : std::string()));
    return (int)OFDM_OK;
}
// ofdm_rx_soft's record, scale table and grid (ofdm_hip_soft.h)
struct RxSoft {
    const double* g;
    double inv_w;
    int32_t bins, k_lo, k_hi;
    uint64_t* hist;
};
// The soft record's own refusals, made before anything else is looked at (p: the plan or null, which
// rx_args then refuses): the arguments, then what of the plan's constellations has no soft form
static int soft_ok(const char* who, const RxSoft& d, ofdm_plan_t p) {
    const auto no = [&](const std::string& why) { return fail(OFDM_E_INVALID, std::string(who) + ": " + why); };
    const int n_fft = p ? p->n : 0;
    if (!d.hist) return no("needs a soft-decision record");
    if (!d.g) return no("needs the subcarriers' scale table g");
    if (d.bins < 2 || d.bins > OFDM_MAX_SOFT_BINS || (d.bins & 1))
        return no("bins " + std::to_string(d.bins) + " is not an even number in [2, " + std::to_string(OFDM_MAX_SOFT_BINS) + "]");
    if (!std::isfinite(d.inv_w) || !(d.inv_w > 0)) return no("inv_w is not a finite positive bin rate");
    if (d.k_lo < 0 || d.k_lo >= d.k_hi || (n_fft > 0 && d.k_hi > n_fft))
        return no("the subcarrier range [" + std::to_string(d.k_lo) + ", " + std::to_string(d.k_hi) +
                  ") is not 0 <= k_lo < k_hi <= n_fft" + (n_fft > 0 ? " = " + std::to_string(n_fft) : std::string()));
    if (p && p->has_const) {
        if (p->wide_plan)
            return no("the plan has a constellation above 256 points, and the soft record of such an order is not built");
        if (!p->separable)
            return no("the plan has a non-separable (PSK) constellation, and the soft record of one is not built "
                      "(square QAM of order 4, 16, 64 or 256 only)");
    }
    return (int)OFDM_OK;
}
// ofdm_rx, ofdm_rx_profile, ofdm_rx_frames, ofdm_rx_density and ofdm_rx_soft (who): the receiver's arguments checked and
// filled, then the entry point's own launch(a, r) -- the filled RxArgs, where the profile sets its record,
// and the plan's precision as a value, float{} or double{} -- answered through checked() (layout_extra: its)
// (extern "C++": a template inside this file's extern "C" block)
extern "C++" template <typename L>
static int rx_call(const char* who, ofdm_plan_t p, const void* y, const double* nr, const double* ni, uint64_t seed,
                   const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on, const uint8_t* bits,
                   int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                   L launch, const std::string& layout_extra = {}) {
    RxArgs a{};
    bool run;
    const int rc = rx_args(who, p, y, nr, ni, seed, stats, total_samples, noise_on, bits, sym0, n_sym, n_valid_bits,
                           counters, [] { return OFDM_OK; }, a, &run);
    if (!run) return rc;
    a.snr_lin = std::pow(10.0, snr_db / 10.0);
    a.z_out = z_out;
    a.z_keep = z_out ? z_keep : 0;
    a.flags = OFDM_ENV_FLAGS("OFDM_ABLATE_RX");
    a.wide = p->wide_plan ? (const WideAxis*)p->wide.p : nullptr;  // an order above 256: the wide slicer
    return checked(who, p, with_prec(p, [&](auto r) { return launch(a, r); }), layout_extra);
}

int ofdm_rx(ofdm_plan_t p, void* stream, const void* y, const double* nr, const double* ni, uint64_t seed,
            const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on, const uint8_t* bits,
            int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters, void* z_out,
            int64_t z_keep) {
    return rx_call("ofdm_rx", p, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits, sym0, n_sym, n_valid_bits,
                   counters, z_out, z_keep, [&](RxArgs& a, auto r) {
                       return launch_rx<decltype(r)>(p->logn, a, (hipStream_t)stream);
                   });
}

int ofdm_rx_profile(ofdm_plan_t p, void* stream, const void* y, const double* nr, const double* ni, uint64_t seed,
                    const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on,
                    const uint8_t* bits, int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters,
                    void* z_out, int64_t z_keep, int64_t* profile) {
    if (!profile) return fail(OFDM_E_INVALID, "ofdm_rx_profile needs a profile record");
    return rx_call("ofdm_rx_profile", p, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits, sym0, n_sym,
                   n_valid_bits, counters, z_out, z_keep, [&](RxArgs& a, auto r) {
                       a.profile = profile;
                       return launch_rx_prof<decltype(r)>(p->logn, a, (hipStream_t)stream);
                   });
}

int ofdm_rx_frames(ofdm_plan_t p, void* stream, const void* y, const double* nr, const double* ni, uint64_t seed,
                   const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on,
                   const uint8_t* bits, int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters,
                   void* z_out, int64_t z_keep, int64_t frame_len, int64_t n_frames, uint64_t* frames) {
    const RxFrames fr{frame_len, n_frames, frames};
    if (const int rc = frames_ok("ofdm_rx_frames", fr, sym0, n_sym)) return rc;
    return rx_call("ofdm_rx_frames", p, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits, sym0, n_sym,
                   n_valid_bits, counters, z_out, z_keep, [&](RxArgs& a, auto r) {
                       return launch_rx_frames<decltype(r)>(p->logn, a, frames_tail(fr, sym0), (hipStream_t)stream);
                   });
}

int ofdm_rx_density(ofdm_plan_t p, void* stream, const void* y, const double* nr, const double* ni, uint64_t seed,
                    const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on,
                    const uint8_t* bits, int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters,
                    void* z_out, int64_t z_keep, double lo, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi,
                    uint64_t* hist) {
    const RxDens dn{lo, inv_w, bins, k_lo, k_hi, hist};
    if (const int rc = dens_ok("ofdm_rx_density", dn, p ? p->n : 0)) return rc;
    RxDensTail d{};  // (flush: the launcher's, by its workgroup shape)
    d.hist = (unsigned long long*)hist;
    d.lo = lo;
    d.inv_w = inv_w;
    d.bins = bins;
    d.k_lo = k_lo;
    d.k_hi = k_hi;
    // (a generic-form layout that does not fit with the histogram: named, nothing was launched)
    return rx_call("ofdm_rx_density", p, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits, sym0, n_sym,
                   n_valid_bits, counters, z_out, z_keep, [&](RxArgs& a, auto r) {
                       return launch_rx_dens<decltype(r)>(p->logn, a, d, (hipStream_t)stream);
                   },
                   " with its " + std::to_string(bins) + " x " + std::to_string(bins) + " density histogram (" +
                       std::to_string(4 * bins * bins) + " bytes)");
}

int ofdm_rx_soft(ofdm_plan_t p, void* stream, const void* y, const double* nr, const double* ni, uint64_t seed,
                 const ofdm_stats* stats, int64_t total_samples, double snr_db, int32_t noise_on, const uint8_t* bits,
                 int64_t sym0, int64_t n_sym, int64_t n_valid_bits, uint64_t* counters, void* z_out, int64_t z_keep,
                 const double* g, double inv_w, int32_t bins, int32_t k_lo, int32_t k_hi, uint64_t* hist) {
    const RxSoft sd{g, inv_w, bins, k_lo, k_hi, hist};
    if (const int rc = soft_ok("ofdm_rx_soft", sd, p)) return rc;
    RxSoftTail t{};  // (flush: the launcher's, by its workgroup shape)
    t.hist = (unsigned long long*)hist;
    t.g = g;
    t.lev = p ? (const double*)p->softlev.p : nullptr;
    t.inv_w = inv_w;
    t.bins = bins;
    t.k_lo = k_lo;
    t.k_hi = k_hi;
    // (a generic-form layout that does not fit with the histogram: named, nothing was launched)
    return rx_call("ofdm_rx_soft", p, y, nr, ni, seed, stats, total_samples, snr_db, noise_on, bits, sym0, n_sym,
                   n_valid_bits, counters, z_out, z_keep, [&](RxArgs& a, auto r) {
                       return launch_rx_soft<decltype(r)>(p->logn, a, t, (hipStream_t)stream);
                   },
                   " with its 20 x 2 x " + std::to_string(bins) + " soft-decision histogram (" +
                       std::to_string(4 * 2 * kSoftRows * bins) + " bytes)");
}

// ofdm_rx_sweep and ofdm_rx_sweep_frames (who; fr: the frame record of every point, or null -- without it
// ofdm_rx_sweep, whose checks, arguments and launch are then what they were)
static int sweep_call(const char* who, ofdm_plan_t p, void* stream, const void* y, uint64_t seed, const ofdm_stats* stats,
                      int64_t total_samples, const double* snr_db, int32_t n_snr, int64_t sym0, int64_t n_sym,
                      int64_t n_valid_bits, uint64_t* counters, const RxFrames* fr = nullptr) {
    const auto points_ok = [&] {
        if (n_snr < 1 || n_snr > OFDM_MAX_SWEEP_POINTS)
            return fail(OFDM_E_INVALID, std::string(who) + " takes 1 to " + std::to_string(OFDM_MAX_SWEEP_POINTS) +
                                            " SNR points per call, got " + std::to_string(n_snr));
        if (!snr_db) return fail(OFDM_E_INVALID, std::string("bad argument to ") + who);
        for (int k = 0; k < n_snr; ++k)
            if (!std::isfinite(snr_db[k]))
                return fail(OFDM_E_INVALID, std::string(who) + ": SNR point " + std::to_string(k) + " is not finite");
        return (int)OFDM_OK;
    };
    RxSweepArgs a{};
    bool run;
    // (Philox streams, noise always on: no caller bits or normals)
    const int rc = rx_args(who, p, y, nullptr, nullptr, seed, stats, total_samples, 1, nullptr, sym0, n_sym,
                           n_valid_bits, counters, points_ok, a.r, &run);
    if (!run) return rc;
    a.n_snr = n_snr;
    for (int k = 0; k < n_snr; ++k) a.snr_lin[k] = std::pow(10.0, snr_db[k] / 10.0);  // (as ofdm_rx)
    a.r.snr_lin = a.snr_lin[0];
    if (fr) {
        const RxFramesTail ft = frames_tail(*fr, sym0);
        return checked(who, p, with_prec(p, [&](auto r) {
            return launch_rx_sweep_frames<decltype(r)>(p->logn, a, ft, (hipStream_t)stream);
        }));
    }
    return checked(who, p, with_prec(p, [&](auto r) {
        return launch_rx_sweep<decltype(r)>(p->logn, a, (hipStream_t)stream);
    }));
}

int ofdm_rx_sweep(ofdm_plan_t p, void* stream, const void* y, uint64_t seed, const ofdm_stats* stats,
                  int64_t total_samples, const double* snr_db, int32_t n_snr, int64_t sym0, int64_t n_sym,
                  int64_t n_valid_bits, uint64_t* counters) {
    return sweep_call("ofdm_rx_sweep", p, stream, y, seed, stats, total_samples, snr_db, n_snr, sym0, n_sym, n_valid_bits,
                      counters);
}

int ofdm_rx_sweep_frames(ofdm_plan_t p, void* stream, const void* y, uint64_t seed, const ofdm_stats* stats,
                         int64_t total_samples, const double* snr_db, int32_t n_snr, int64_t sym0, int64_t n_sym,
                         int64_t n_valid_bits, uint64_t* counters, int64_t frame_len, int64_t n_frames,
                         uint64_t* frames) {
    // (n_frames: the rows of one point; the record holds n_snr times as many)
    const RxFrames fr{frame_len, n_frames, frames};
    if (const int rc = frames_ok("ofdm_rx_sweep_frames", fr, sym0, n_sym)) return rc;
    return sweep_call("ofdm_rx_sweep_frames", p, stream, y, seed, stats, total_samples, snr_db, n_snr, sym0, n_sym,
                      n_valid_bits, counters, &fr);
}

// ofdm_link, ofdm_link_sparse, ofdm_link_nscreen and ofdm_link_screen (screen: the kernel's, kLinkScreen*;
// mode, screen_counts: the screen's)
static int link_call(int screen, ofdm_plan_t p, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
                     double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
                     uint64_t* counters, int32_t mode, uint64_t* screen_counts) {
    // what has a fused form, each refusal naming its reason (the launcher's link_shape holds the same
    // conditions on the kernel's arguments); never another path in its place
    const auto fused_form = [&] {
        const auto no = [](const std::string& why) {
            return fail(OFDM_E_INVALID, "ofdm_link: no fused form: " + why + "; use ofdm_tx and ofdm_rx");
        };
        if (p->prec != OFDM_F64) return no("the plan is complex64");
        if (p->L != 1) return no("the channel has " + std::to_string(p->L) + " taps (flat channels only)");
        if (p->eq != OFDM_EQ_NONE) return no("the plan has an equaliser");
        if (p->n != 1024 || p->adaptive || !p->separable || p->psk_m != 0 || p->b != 6 || p->single_carrier ||
            (p->zp && p->cp > 0))
            return no("the plan is not fixed 64-QAM cyclic-prefix OFDM at n_fft 1024");
        // (the fixed-order receivers compare every bit and ignore n_valid_bits: a shorter count
        // cannot be honoured here)
        if (n_sym > 0 && n_valid_bits < (sym0 + n_sym) * (int64_t)p->bps)
            return no("n_valid_bits " + std::to_string(n_valid_bits) + " is short of the call's " +
                      std::to_string((sym0 + n_sym) * (int64_t)p->bps) + " bits");
        return (int)OFDM_OK;
    };
    LinkArgs a{};
    bool run;
    // (Philox streams, no y: the registers carry it; rx_args wants a non-null y, never read)
    const int rc = rx_args("ofdm_link", p, counters, nullptr, nullptr, seed, stats, total_samples, noise_on, nullptr,
                           sym0, n_sym, n_valid_bits, counters, fused_form, a.r, &run);
    if (!run) return rc;
    a.r.y = nullptr;
    a.r.snr_lin = std::pow(10.0, snr_db / 10.0);
    a.r.flags = OFDM_ENV_FLAGS("OFDM_ABLATE_RX");  // (8: the noise screen without its add and slicer; ablation builds)
    a.h = p->h.p;
    a.mode = mode;
    a.screen_counts = (unsigned long long*)screen_counts;
    return checked("ofdm_link", p, launch_link<double>(p->logn, p->L, a, screen, (hipStream_t)stream));
}

// the mode of the entry points that take one (name: the entry point's, for the message)
static int link_mode_ok(const char* name, int32_t mode) {
    if (mode == OFDM_LINK_SCREEN_AUTO || mode == OFDM_LINK_SCREEN_OFF || mode == OFDM_LINK_SCREEN_FORCED) return OFDM_OK;
    return fail(OFDM_E_INVALID, std::string(name) + ": mode " + std::to_string(mode) + " is not an OFDM_LINK_SCREEN_* value");
}

int ofdm_link(ofdm_plan_t p, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
              double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
              uint64_t* counters) {
    return link_call(kLinkScreenSparse, p, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid_bits,
                     counters, OFDM_LINK_SCREEN_AUTO, nullptr);
}

int ofdm_link_sparse(ofdm_plan_t p, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
                     double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
                     uint64_t* counters, int32_t mode, uint64_t* sparse_counts) {
    if (const int rc = link_mode_ok("ofdm_link_sparse", mode)) return rc;
    // off: the noise screen itself in its automatic mode, and nothing counted
    if (mode == OFDM_LINK_SCREEN_OFF)
        return link_call(kLinkScreenNoise, p, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid_bits,
                         counters, OFDM_LINK_SCREEN_AUTO, nullptr);
    return link_call(kLinkScreenSparse, p, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid_bits,
                     counters, mode, sparse_counts);
}

int ofdm_link_nscreen(ofdm_plan_t p, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
                      double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
                      uint64_t* counters, int32_t mode, uint64_t* screen_counts) {
    if (const int rc = link_mode_ok("ofdm_link_nscreen", mode)) return rc;
    return link_call(kLinkScreenNoise, p, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid_bits,
                     counters, mode, screen_counts);
}

int ofdm_link_screen(ofdm_plan_t p, void* stream, uint64_t seed, const ofdm_stats* stats, int64_t total_samples,
                     double snr_db, int32_t noise_on, int64_t sym0, int64_t n_sym, int64_t n_valid_bits,
                     uint64_t* counters, int32_t mode, uint64_t* screen_counts) {
    if (const int rc = link_mode_ok("ofdm_link_screen", mode)) return rc;
    return link_call(kLinkScreenTwo, p, stream, seed, stats, total_samples, snr_db, noise_on, sym0, n_sym, n_valid_bits,
                     counters, mode, screen_counts);
}

int ofdm_papr(ofdm_plan_t p, void* stream, const uint8_t* bits, uint64_t seed, int64_t sym0, int64_t n_sym,
              const double* edges, int32_t n_edges, uint64_t* hist, double* sym_out, int64_t sym_keep) {
    if (!p || !p->has_const) return fail(OFDM_E_INVALID, "ofdm_papr needs a constellation");
    if (n_sym < 0 || sym0 < 0 || !hist) return fail(OFDM_E_INVALID, "bad argument to ofdm_papr");
    if (int rc = symbols_ok("ofdm_papr", sym0, n_sym)) return rc;
    if (n_edges < 1 || n_edges > OFDM_MAX_PAPR_EDGES)
        return fail(OFDM_E_INVALID, "ofdm_papr takes 1 to " + std::to_string(OFDM_MAX_PAPR_EDGES) +
                                        " edges per call, got " + std::to_string(n_edges));
    if (!edges) return fail(OFDM_E_INVALID, "bad argument to ofdm_papr");
    for (int k = 0; k < n_edges; ++k) {
        if (!std::isfinite(edges[k]) || !(edges[k] > 0.0))
            return fail(OFDM_E_INVALID, "ofdm_papr: edge " + std::to_string(k) + " is not a finite positive ratio");
        if (k > 0 && !(edges[k] > edges[k - 1]))
            return fail(OFDM_E_INVALID, "ofdm_papr: edge " + std::to_string(k) + " is not above its predecessor "
                                        "(the edges must be strictly increasing)");
    }
    if (int rc = stream_bits_ok(p, bits, "ofdm_papr")) return rc;
    // (after stream_bits_ok: without caller bits a wide plan answers as ofdm_tx does)
    if (p->wide_plan)
        return fail(OFDM_E_INVALID, "ofdm_papr: the plan has a constellation above 256 points, and the wide map is "
                                    "not built into k_papr (orders up to 256 only)");
    if (n_sym == 0) return OFDM_OK;
    PaprArgs a{};
    a.n_edges = n_edges;
    std::memcpy(a.edges, edges, sizeof(double) * (size_t)n_edges);
    // a workgroup counts its symbols in 32-bit bins: launches of at most 2^31 symbols
    const int64_t kMaxLaunch = (int64_t)1 << 31;
    for (int64_t done = 0; done < n_sym; done += kMaxLaunch) {
        const int64_t n = std::min(kMaxLaunch, n_sym - done);
        // the bits buffer covers global symbols [0, sym0 + n_sym)
        fill_common(p, a.c, bits, seed, sym0 + done, n, sym0 + n_sym);
        a.hist = (unsigned long long*)hist;
        a.sym_out = (sym_out && sym_keep > done) ? sym_out + 2 * done : nullptr;
        a.sym_keep = a.sym_out ? sym_keep - done : 0;
        if (int rc = checked("ofdm_papr", p, with_prec(p, [&](auto r) {
                return launch_papr<decltype(r)>(p->logn, a, (hipStream_t)stream);
            })))
            return rc;
    }
    return OFDM_OK;
}

}  // extern "C"
