// ofdm_link_inst.hpp -- the fused link kernel k_link (ofdm_link) and its launcher; included by
// ofdm_kernels_f64_link.hip, a translation unit of its own beside the k_tx / k_rx / k_rx_prof /
// k_rx_sweep ones (every other object stays as it was).
//
// k_link transmits and receives a symbol in one wave without the kept channel samples y leaving the
// registers: the flat transmitter's sequence (lane block -> LUT gather -> IFFT: the statements of
// k_tx<double, LOGN, FB, 0> on the same templates, in the same order, so the registers hold the values
// k_tx would have stored) and then the no-equaliser receiver's body on them in place of its buffer
// loads (add_noise64 -> FFT -> slicer -> XOR / popcount -> the u64 atomics: ofdm_rx_body.hpp's
// statements for F64_FAST, EQ = NONE, MV = false).  The lane's Philox block is drawn once and serves
// both halves.  No y store, no y load, no statistics: the power the noise is scaled by, sum |x|^2 and
// the peak come from the power pass (ofdm_tx with y = NULL) over the whole stream.
//
// Shape: complex128, fixed square QAM of FB bits, cyclic-prefix OFDM (or no prefix), flat channel,
// Philox streams, no equaliser -- bench config (b) at N = 1024, FB = 6.
//
// SCREEN = kLinkScreenTwo (ofdm_link_screen): the kernel reports integer decisions only, and a
// decision needs complex128 only when the received point lies within rounding distance of a slicer
// boundary.  Each wave first runs its symbol in float32 on the complex64 kernels' templates (the float
// LUT gather, fft_sym<float>, Mwc64x::add_noise, PermSlicer's two packed FMAs) and proves, per element
// and axis, that the level coordinate is further from every half-integer boundary than delta, a
// rigorous bound on the distance between the float32 and the float64 coordinate of this symbol
// (screen_bound below).  One ballot: every element decisive -> the float32 XOR /
// popcount is the symbol's count (the levels are the float64 path's, so the words are); otherwise the
// wave re-seeds and redoes the whole symbol on the complex128 statements, unchanged.  The counts are
// the unscreened kernel's whatever share is redone.
//
// SCREEN = kLinkScreenNoise (ofdm_link's automatic mode, ofdm_link_nscreen): the channel is one tap folded
// into the LUT and nothing is done to the prefix, so in exact arithmetic the spectrum the slicer sees is
// z_k = N l_k + G_k, l the folded LUT entry of subcarrier k and G the unnormalised FFT of the symbol's
// noise: the IFFT and the FFT of its output only reproduce N l_k, a number already in LDS.  The noise
// screen transforms the noise alone in float32 (one transform, forward twiddles only) and adds the LUT
// point scaled by N (exact: N is a power of two) per element -- element i of a lane is subcarrier byte i
// of the lane block on the way in and on the way out.  Its bound scales with the noise, not the signal
// (nscreen_const below); the ballot, the counts and the redo are the same.
//
// SCREEN = kLinkScreenSparse (ofdm_link's automatic mode, ofdm_link_sparse): the noise screen, slicing only
// the quads the noise can reach.  Before the point is added xf holds the bare ghat, and a quad (elements
// 4q .. 4q+3 of every lane) none of whose 512 components exceeds T in modulus provably gives the
// transmitted levels and a margin inside thr (sparse_eps below): its difference word
// is 0 and it leaves m <= thr, so the add, diff_margin and the counts are skipped for it -- one max3
// chain and a ballot per quad.  The counts, the symbols redone and the screen's counts are the noise
// screen's for every input.  Whether a launch tests its quads or runs the noise screen's unrolled
// sequence is a workgroup-uniform decision beside `screen` (sparse_mu below).
//
// The three screens share their text: one prologue (the tables, the slicer, the constants and the decision;
// the sparse part behind it), one quad-slicing statement (`slice` in the screened symbol, called per tested
// quad or for all four), one table-point add (AddPoint) and one undecided-axes formula (undecided_axes).
// SCREEN = none, Two and Noise compile to the instructions they had with a copy each
// (profiles/link_refactor_kernel_audit.txt); the symbol loop stays inline for the same reason -- a lambda
// or a function around the screened symbol, even one never called, moves all four kernels' registers.
//
// The screens also share the wave sum of the norm (wave_sum_f32: DPP and lane swaps, no LDS), so that the
// sparse form's delta, and with it the symbols it redoes, stay the noise screen's.  The sparse form alone has
// the max3 maxima (the quad test and the margin, max_abs2 / max_abs3) and its own copy of the generator step
// for the screened symbol's noise (ScreenMwc): Two and Noise differ from their earlier code by the sum only,
// none not at all (profiles/link_trim_kernel_audit.txt).
#pragma once

#include "ofdm_kernels_inst.hpp"

namespace ofdm {

// The workgroup: both transforms' per-pass twiddles (the inverse ones are the forward ones' exact
// conjugates, held as the plan uploads them: [forward | inverse]) and the LUT beside the rows leave
// room for 12 symbols' rows of reals, not the receiver's 16 -- 768 threads, 3 waves per SIMD
// (168 VGPRs: nothing spilled, where the 1024-thread receiver spills 6 dwords at 128).
#ifndef OFDM_LINK_BLOCK
#define OFDM_LINK_BLOCK 768
#endif
#ifndef OFDM_LINK_WAVES
#define OFDM_LINK_WAVES 3
#endif
// OFDM_LINK_NOREDO (ablation builds only, with OFDM_LINK_BLOCK=1024 and OFDM_LINK_WAVES=4): the sparse form
// without its complex128 redo and that redo's tables (the double twiddles and LUT staged through the rows,
// no ntab64) -- the ceiling of a float32-only screen kernel.  A timing build: an undecided symbol is
// counted from its float32 words, and the other instantiations are not meant to be launched from it.
#if OFDM_ABLATION && defined(OFDM_LINK_NOREDO)
constexpr bool link_noredo(int screen) { return screen == kLinkScreenSparse; }
#else
constexpr bool link_noredo(int) { return false; }
#endif

// (k_link's SCREEN -- kLinkScreenNone, Two, Noise, Sparse -- is ofdm_launch.hpp's: the ABI names one)

template <typename R>
struct LinkLds {
    cpx<R>* tt;  // per-pass twiddles [forward | inverse]
    AxisInfo* axis;
    unsigned char* rowmem;
    unsigned long long* redc;
    // kLinkScreenTwo: the same twiddles [forward | inverse] and the folded LUT rounded to float32;
    // kLinkScreenNoise, kLinkScreenSparse: the forward twiddles only, and that LUT times N
    cpx<float>* tt32;
    cpx<float>* lut32;
};
template <typename R, int LOGN, int SCREEN = kLinkScreenNone, int FB = 0, typename CV>
__host__ __device__ __forceinline__ constexpr LinkLds<R> link_carve(CV& cv) {
    using G = Geo<LOGN, OFDM_LINK_BLOCK>;
    LinkLds<R> m{};
    m.axis = cv.template take<AxisInfo>(kMaxLuts);
    // (PADN complex64 take what PADN doubles take: the float32 transforms exchange through the same row)
    m.rowmem = cv.template take<unsigned char>((size_t)G::SPB * G::PADN * sizeof(R));
    m.redc = cv.template take<unsigned long long>(OFDM_LINK_BLOCK / 64);
    m.tt = cv.template take<cpx<R>>(link_noredo(SCREEN) ? 0 : 2 * tt_size(LOGN));
    m.tt32 = cv.template take<cpx<float>>(SCREEN == kLinkScreenTwo ? 2 * tt_size(LOGN) : SCREEN ? tt_size(LOGN) : 0);
    m.lut32 = cv.template take<cpx<float>>(SCREEN ? (1 << FB) : 0);
    return m;
}
// static LDS: the transmitter's LUT, the noise phase table and its widening to double
template <typename R, int FB>
constexpr size_t link_static_lds() { return (1 << FB) * sizeof(cpx<R>) + rx_static_lds<R, FB>(); }

// ---- the screen's bound (DESIGN.md section 4 has the derivation)
// u = 2^-24, the float32 unit roundoff.  Higham, Accuracy and Stability of Numerical Algorithms, Theorem
// 24.2: a transform of t = log2 N radix-2 levels with twiddles off by mu has a relative 2-norm error
// of at most t eta / (1 - t eta), eta = mu + gamma_4 (sqrt 2 + mu).  The 16.16.4 passes are 10 such
// levels with fewer products than radix 2 has (4 on a path), and the twiddles, the w16 constants and
// the LUT are float64 values rounded once (mu <= u): eta <= 6.66 u, 66.6 u per transform.  With the
// LUT's rounding and the noise FMA's (one u each) the received spectrum z of a symbol obeys
//   |z32_k - z64_k| <= ||z32 - z64||_2 <= kScreenK u (||z32||_2 + sqrt N ||x||_2),  kScreenK = 70,
// x the transmitted samples, ||x||_2 <= N a with a the largest modulus of the folded LUT (1 / sqrt N
// inside); 70 over 67.6 covers the 1 / (1 - t eta), the second-order terms, the float64 side's 2^-53
// ones and the float32 evaluation of the norm and of this bound.
constexpr double kScreenK = 70.0;
constexpr double kScreenU = 0x1p-24;
// the level coordinate's own roundings, in levels: the slicer's two constants and its first FMA
// ((0.6 + 0.5 + 1) u of the clamped coordinate, times side - 1 <= 15), and the margin's FMA
constexpr double kScreenSlicerU = 40.0;
// automatic mode: screen when the expected number of undecided axes of a symbol is below this (a
// share 1 - exp(-0.35) = 0.30 of the symbols redone; the screen pays below about 0.4)
constexpr double kScreenMaxUndecided = 0.35;

// The sparse form's largest moduli (the quad test's components, the margin's two axes): v_max_f32 / v_max3_f32
// on the |.| source modifiers, one instruction per element.  fmaxf of two fabsf quiets each operand first (a
// v_max_f32 |a|, |a| apiece); these return the same number for every input that is not a NaN, and drop a NaN
// as fmaxf does -- the kernel says what becomes of a symbol with one.
__device__ __forceinline__ float max_abs2(f32x2 a) {
    float r;
    asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a.x), "v"(a.y));
    return r;
}
__device__ __forceinline__ float max_abs3(f32x2 a, float mx) {
    float r;
    asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a.x), "v"(a.y), "v"(mx));
    return r;
}

// PermSlicer with the decision's margin: m = max(m, |y - round(y)|) over both axes of the four elements,
// y the clamped level coordinate -- 1/2 - m is the distance to the nearest decision boundary (a clamped
// end gives y = round(y): never near one).
template <int FB>
struct ScreenSlicer : PermSlicer<FB> {
    using P = PermSlicer<FB>;
    __device__ void load(const AxisInfo& a, double scale) {
        P::load(a, (float)scale);
        // the level multiplier rounded once from the double product (P::load rounds the scale first)
        const float is = (float)(a.inv_step * scale / (double)(P::SIDE - 1));
        this->mul = f32x2{is, is};
    }
    // MAX3: the margin through max_abs3 (the sparse form; the other screens keep their instructions)
    template <bool MAX3 = false>
    __device__ __forceinline__ uint32_t diff_margin(const cpx<float> (&z)[4], uint32_t txw, float& m) const {
        uint32_t li[4], lq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x2 v;
            asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(v) : "v"(z[j].v), "v"(this->mul), "v"(this->add));
            uint64_t fb;
            asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(fb) : "v"(v), "v"(this->smax), "v"(this->magic));
            li[j] = (uint32_t)fb;
            lq[j] = (uint32_t)(fb >> 32);
            // round(y) = the magic sum less the magic, exact; y - round(y) in one FMA, per axis in
            // scalar float (no lane of a packed value is reinterpreted)
            const float ri = __uint_as_float(li[j]) - 12582912.0f, rq = __uint_as_float(lq[j]) - 12582912.0f;
            const float ei = __builtin_fmaf(v.x, this->smax.x, -ri), eq = __builtin_fmaf(v.y, this->smax.x, -rq);
            if constexpr (MAX3) m = max_abs3(f32x2{ei, eq}, m);
            else m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(ei), __builtin_fabsf(eq)));
        }
        const uint32_t si = __builtin_amdgcn_perm(__builtin_amdgcn_perm(li[3], li[2], 0x0c0c0400u),
                                                  __builtin_amdgcn_perm(li[1], li[0], 0x0c0c0400u), 0x05040100u);
        const uint32_t sq = __builtin_amdgcn_perm(__builtin_amdgcn_perm(lq[3], lq[2], 0x0c0c0400u),
                                                  __builtin_amdgcn_perm(lq[1], lq[0], 0x0c0c0400u), 0x05040100u);
        return (P::lookup(this->ti, si) | P::lookup(this->tq, sq)) ^ (txw & P::BYTE_MASK);
    }
};

// The screen's constants of a launch: delta in levels = cz ||z32||_2 + c0 (screen_bound above times
// the level multiplier, plus the slicer's own roundings), and, under noise, delta at the expected norm and
// the expected undecided axes per symbol there.
struct ScreenConst {
    float cz, c0;
    double delta = 0.0, undecided = 0.0;
    // kz, k0: the two constants in double (1.001: the float rounding of the two and of cz sqrt(n2) + c0 itself)
    __host__ __device__ ScreenConst(double kz, double k0) : cz((float)(1.001 * kz)), c0((float)(1.001 * k0)) {}
};
// An axis is undecided when its coordinate lies within delta of one of the side - 1 boundaries; under noise
// of deviation sc levels the coordinate's density there is phi(1/2 / sc) / sc from each of the two levels
// beside it, each sent with probability 1 / side.
template <int LOGN, int FB>
__host__ __device__ inline double undecided_axes(double delta, double sc) {
    constexpr double N = (double)(1 << LOGN), side = (double)(1 << (FB / 2));
    const double phi = exp(-0.125 / (sc * sc)) * 0.3989422804014327 / sc;
    return 2.0 * N * (side - 1.0) * (2.0 / side) * 2.0 * delta * phi;
}
// lvl: levels per unit of z (the slicer's multiplier times side - 1); amax: the folded LUT's largest
// modulus; p: the stream's mean sample power; sigma: the noise's per-component deviation
template <int LOGN, int FB>
__host__ __device__ inline ScreenConst screen_const(double lvl, double amax, double p, double sigma) {
    constexpr double N = (double)(1 << LOGN);
    const double rootn = sqrt(N);
    const double kz = kScreenK * kScreenU * lvl;
    ScreenConst c(kz, kz * N * rootn * amax + kScreenSlicerU * kScreenU);
    if (sigma > 0.0) {  // ||z||_2 ~ N sqrt(p + 2 sigma^2)
        const double sc = sigma * rootn * lvl;
        c.delta = kz * (N * sqrt(p + 2.0 * sigma * sigma) + N * rootn * amax) + kScreenSlicerU * kScreenU;
        c.undecided = undecided_axes<LOGN, FB>(c.delta, sc);
    }
    return c;
}

// ---- the noise screen's bound
// zhat_k = fl(N l32_k + ghat_k), ghat the float32 transform of nhat = fl(r e), the once-rounded float32
// product the complex128 kernel takes exactly.  ||nhat - n||_2 <= u ||n||_2, so by the theorem above and
// linearity ||ghat - G||_2 <= (66.6 + 1) u ||G||_2 (1 + O(u)); the LUT's rounding is u N a, the final
// add's u (N a + |ghat_k|), the complex128 kernel's own two transforms 70 2^-53 (2 N^1.5 a + ||G||_2),
// below 1e-3 u N a.  With |ghat_k| <= ||ghat||_2 and ||G||_2 <= ||ghat||_2 (1 + 68 u):
//   |zhat_k - z64_k| <= kNScreenK u ||ghat||_2 + kNScreenC u N a,  kNScreenK = 72, kNScreenC = 3;
// 72 over 68.6 and 3 over 2 cover the 1 / (1 - t eta), the second-order terms, the float64 side and the
// float32 evaluation of the norm and of this bound.
constexpr double kNScreenK = 72.0;
constexpr double kNScreenC = 3.0;
// automatic mode: a screened symbol costs about half a complex128 one, so the screen pays up to about
// half of the symbols redone.  Measured (profiles/link_nscreen_ab.txt): forced wins down to 8 dB (0.46
// redone, lambda below 0.487) and loses from 6 dB (0.53 redone, lambda 0.513); lambda counts the two levels
// beside a boundary only and so saturates at low SNR, where the shares redone keep growing
constexpr double kNScreenMaxUndecided = 0.5;

// delta in levels = cz ||ghat||_2 + c0, and the expected undecided axes per symbol (||ghat||_2 ~ N sigma sqrt 2)
template <int LOGN, int FB>
__host__ __device__ inline ScreenConst nscreen_const(double lvl, double amax, double sigma) {
    constexpr double N = (double)(1 << LOGN);
    const double kz = kNScreenK * kScreenU * lvl;
    const double k0 = kNScreenC * kScreenU * lvl * N * amax + kScreenSlicerU * kScreenU;
    ScreenConst c(kz, k0);
    if (sigma > 0.0) {
        const double sc = sigma * sqrt(N) * lvl;
        c.delta = kz * N * sigma * 1.4142135623730951 + k0;
        c.undecided = undecided_axes<LOGN, FB>(c.delta, sc);
    }
    return c;
}

// ---- the sparse slicer's threshold
// A skipped quad must be one for which diff_margin returns 0 and leaves m <= thr.  In levels, with k the
// table point's own level on an axis, rho = |p lvl + off - k| the point's own distance from it under the
// slicer's float32 constants (taken from the table in the prologue, so neither constant's rounding needs a
// bound), c = ghat lvl and S the side: the final add moves the coordinate by at most u S / 2, the first
// FMA by u (S - 1/2), the clamp moves it towards [0, S - 1], which holds k, the magic sum rounds the exact
// product v (S - 1) to the nearest integer (so the level is k while the distance is below 1/2), the
// margin's FMA adds u / 2, thr = fl(1/2 - delta) is off by u / 4 and T = fl(fl(thr - e0) fl(1 / lvl)) by
// 1.25 u of a level: (1.5 S + 1.5) u in all.  eps = (1.5 S + 6) u leaves 4.5 u for the second-order terms
// and the double evaluation of rho; e0 = 1.001 (eps + rho) covers its own rounding to float32.
//   |ghat component| <= T = (thr - e0) / lvl for all eight of a quad in every lane  =>  d = 0, m_quad <= thr.
constexpr double sparse_eps(int side) { return (1.5 * side + 6.0) * kScreenU; }
// automatic mode: test the quads when the expected number of components over T per quad index and wave
// is below this (a share 1 - exp(-mu) of the quads sliced).  Measured (profiles/link_sparse_ab.txt): the
// forced test wins down to 23 dB (mu = 1.05, 0.65 of the quads sliced: 1.654 against 1.706 ms) and loses
// from 22 dB (mu = 3.1, 0.95 sliced: 1.811 against 1.729) -- a sliced quad pays its test and the branch
constexpr double kSparseMaxPerQuad = 2.0;
// mu = 8 * 64 * 2 Q(T_levels / sigma_c): sigma_c the noise's deviation per component in levels, T_levels at
// delta, nscreen_const's at the expected norm ||ghat||_2 ~ N sigma sqrt 2; no room under 1/2: every quad
template <int LOGN, int FB>
__host__ __device__ inline double sparse_mu(double lvl, double sigma, double delta, double rho) {
    if (!(sigma > 0.0)) return 0.0;
    const double t = 0.5 - delta - 1.001 * (sparse_eps(1 << (FB / 2)) + rho);
    const double sc = sigma * sqrt((double)(1 << LOGN)) * lvl;
    return t > 0.0 ? 512.0 * erfc(t / (sc * 1.4142135623730951)) : 512.0;
}

// a wave's quads tested and sliced (wave-uniform; a wave's symbols: far below 2^32), and nothing at all in
// the instantiations that test none
template <bool SPARSE>
struct QuadCounts {};
template <>
struct QuadCounts<true> {
    unsigned tested = 0, sliced = 0;
};

// the noise screens: xf[I] += the table point N l32 of element I's subcarrier (static_for's body)
template <int E, typename TB>
struct AddPoint {
    cpx<float> (&xf)[E];
    const cpx<float>* lut32;
    const TB& tb;
    template <typename I>
    __device__ __forceinline__ void operator()(I) const { xf[I::value].v += lut32[tb.template fixed<I::value>()].v; }
};

// The screens' wave sum of a float (the norm ||ghat||^2), the same bits in every lane, without LDS: four DPP
// adds inside a row of 16 lanes (lane ^ 1, lane ^ 2, then the row's half and whole mirrors, every lane of a
// quad and of a half row already holding the same partial sum), then the rows through v_permlane16_swap
// and v_permlane32_swap of the value with itself -- where __shfl_xor is six ds_bpermute round trips.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_sum_f32(float v) {
    v += dpp_f32<0xB1>(v);   // quad_perm:[1,0,3,2]
    v += dpp_f32<0x4E>(v);   // quad_perm:[2,3,0,1]
    v += dpp_f32<0x141>(v);  // row_half_mirror
    v += dpp_f32<0x140>(v);  // row_mirror
    const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);  // rows 0 + 1 | rows 2 + 3
    const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
}

// The sparse form's copy of the lane generator for the screened symbol's noise: Mwc64x's outputs, word for
// word (tests/test_oracle_philox.py pins the stream), with the carry held zero-extended so that a step is
// the v_mad_u64_u32 onto that pair and one v_lshrrev_b64 of the product -- where (x, c) in two words costs
// two v_mov_b32 a step to rebuild the addend (c, 0).  The shared generator and every other kernel stay.
struct ScreenMwc {
    uint32_t x, q;
    uint64_t cz;  // the carry c, its high word 0
    __device__ __forceinline__ explicit ScreenMwc(const Mwc64x& g) : x(g.x), q(0), cz(g.c) {}
    __device__ __forceinline__ uint32_t next() {
        const uint32_t r = x ^ (uint32_t)cz;
        const uint64_t v = (uint64_t)kMwcA * x + cz;
        x = (uint32_t)v;
        asm("v_lshrrev_b64 %0, 32, %1" : "=v"(cz) : "v"(v));
        return r;
    }
    // Mwc64x::add_noise: the phase word before samples 0 mod 4, the radius word, one packed FMA
    __device__ __forceinline__ void add_noise(f32x2& x0, const f32x2* ntab, int j) {
        if ((j & 3) == 0) q = next();
        const float r = noise_radius(next());
        const uint32_t off = ((q >> (8 * (j & 3))) & (uint32_t)(kNoisePhases - 1)) * (uint32_t)sizeof(f32x2);
        const f32x2 e = *(const f32x2*)((const unsigned char*)ntab + off);
        x0 = __builtin_elementwise_fma(f32x2{r, r}, e, x0);
    }
};

template <typename R, int LOGN, int FB, int SCREEN = kLinkScreenNone>
__global__ __launch_bounds__(OFDM_LINK_BLOCK, OFDM_LINK_WAVES) void k_link(LinkArgs la) {
    static_assert(sizeof(R) == 8 && FB > 1 && !(FB & 1), "complex128 fixed square QAM");
    static_assert(uses_tt<R, LOGN, FB>() && Geo<LOGN>::TPS >= 64, "a symbol per wave, per-pass twiddles in LDS");
    static_assert(!SCREEN || Geo<LOGN>::TPS == 64, "the screen's ballot and its redo are one wave's");
    constexpr bool NOISE_ALONE = SCREEN == kLinkScreenNoise || SCREEN == kLinkScreenSparse;
    constexpr bool SPARSE = SCREEN == kLinkScreenSparse;
    constexpr bool NOREDO = link_noredo(SCREEN);
    constexpr int BLK = OFDM_LINK_BLOCK;
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr int E = G::E, TPS = G::TPS;
    constexpr int TTS = tt_size(LOGN);
    const RxArgs& a = la.r;
    const TxRxCommon& cm = a.c;
    __shared__ C lut_s[1 << FB];
    __shared__ f32x2 ntab[kNoisePhases];
    __shared__ f64x2 ntab64[kNoisePhases];
    Carve cv(ofdm_smem);
    const LinkLds<R> lds = link_carve<R, LOGN, SCREEN, FB>(cv);
    C* tt = NOREDO ? (C*)lds.rowmem : lds.tt;
    C* const lutd = NOREDO ? tt + 2 * TTS : lut_s;
    AxisInfo* axis = lds.axis;
    unsigned long long* redc = lds.redc;

    // the tables' global reads issued first (Staged), the noise table built while they fly
    Staged<BLK, 2 * TTS, C> st_tt;
    Staged<BLK, (1 << FB), C, true> st_lut;
    Staged<BLK, kMaxLuts, Dwords<AxisInfo>> st_ax;
    static_assert(kMaxLuts <= BLK, "one axis entry per thread");
    const C hf = ((const C*)la.h)[0];
    st_tt.load((const C*)cm.ptw, 2 * TTS);
    st_lut.load((const C*)cm.lut, cm.lut_len);
    st_ax.load((const Dwords<AxisInfo>*)cm.axis, cm.n_axis);
    // sigma from the whole-stream mean power (as k_rx)
    const bool noise = a.noise_on;
    double sigma_d = 0;
    [[maybe_unused]] double power = 0;
    if (noise) {
        const double p = a.stats[0] / (double)a.total_samples;
        sigma_d = sqrt((p / a.snr_lin) / 2.0);
        power = p;
    }
    build_noise_table(ntab, sigma_d, NOREDO ? nullptr : ntab64);
    st_tt.store(tt);
    // the 1/sqrt(N) of ifft(norm="ortho") and the channel tap folded into the LUT (as k_tx, FOLD_H0)
    const R lut_scale = (R)cm.scale;
    st_lut.store(lutd, [&](const C& v) { return cscale(cmul(hf, v), lut_scale); });
    st_ax.store((Dwords<AxisInfo>*)axis);
    __syncthreads();

    const int ls = __builtin_amdgcn_readfirstlane(threadIdx.x / TPS);
    const int t = threadIdx.x % TPS;
    C* row = (C*)(lds.rowmem + (size_t)ls * G::PADN * sizeof(R));
    PermSlicer64<FB> pslicer;
    pslicer.load(axis[0], cm.scale);  // the FFT output stays unscaled (x sqrt N)

    // SCREEN: the float32 tables rounded from the staged double ones (what a complex64 plan uploads;
    // the LUT from the folded one), the slicer, the bound's constants and the workgroup's decision
    using CF = cpx<float>;
    [[maybe_unused]] CF* const tt32 = lds.tt32;
    [[maybe_unused]] CF* const lut32 = lds.lut32;
    [[maybe_unused]] ScreenSlicer<FB> fslicer;
    [[maybe_unused]] bool screen = false;
    [[maybe_unused]] float cz = 0, c0 = 0;
    // kLinkScreenSparse: test each quad against T = (thr - e0) inv_lvl, or slice them all (the noise screen)
    [[maybe_unused]] bool sparse = false;
    [[maybe_unused]] float e0 = 0, inv_lvl = 0;
    [[maybe_unused]] QuadCounts<SPARSE> quads;
    if constexpr (SCREEN) {
        // kLinkScreenTwo: both twiddle tables and the LUT as it is; the noise screens: the forward twiddles
        // only, and the LUT times N (a power of two: the same rounding)
        constexpr int SIDE = PermSlicer<FB>::SIDE;
        constexpr float POINT = NOISE_ALONE ? (float)(1 << LOGN) : 1.f;
        for (int i = threadIdx.x; i < (NOISE_ALONE ? 1 : 2) * TTS; i += BLK) tt32[i] = mk<float>((float)tt[i].re, (float)tt[i].im);
        double amax = 0;
        for (int i = 0; i < (1 << FB); ++i) {
            const C v = lutd[i];
            amax = fmax(amax, v.re * v.re + v.im * v.im);
            if (i == (int)threadIdx.x) lut32[i] = mk<float>(POINT * (float)v.re, POINT * (float)v.im);
        }
        static_assert((1 << FB) <= BLK, "one LUT entry per thread");
        fslicer.load(axis[0], cm.scale);
        const double lvl = (double)fslicer.mul.x * (double)(SIDE - 1);
        const ScreenConst sc = NOISE_ALONE ? nscreen_const<LOGN, FB>(lvl, sqrt(amax), sigma_d)
                                           : screen_const<LOGN, FB>(lvl, sqrt(amax), power, sigma_d);
        cz = sc.cz;
        c0 = sc.c0;
        screen = la.mode == OFDM_LINK_SCREEN_FORCED || !noise ||
                 sc.undecided < (NOISE_ALONE ? kNScreenMaxUndecided : kScreenMaxUndecided);
        __syncthreads();
        if constexpr (SPARSE) {
            // rho: the largest distance of a table point from its own level under the slicer's constants,
            // in double from the float32 values the screen adds and multiplies by -- lane e takes entry e
            // (every wave the same); a point whose bits no level carries leaves no T at all
            const double offl = (double)fslicer.add.x * (double)(SIDE - 1);
            double rho = 0;
            for (int e = threadIdx.x % 64; e < (1 << FB); e += 64) {
                const double pi = (double)lut32[e].re, pq = (double)lut32[e].im;
                double ri = 1.0, rq = 1.0;
                for (int k = 0; k < SIDE; ++k) {
                    if (axis[0].ipat[k] == (e & (SIDE - 1))) ri = fabs(fma(pi, lvl, offl) - (double)k);
                    if (axis[0].qpat[k] == (e >> (FB / 2))) rq = fabs(fma(pq, lvl, offl) - (double)k);
                }
                rho = fmax(rho, fmax(ri, rq));
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) rho = fmax(rho, __shfl_xor(rho, off, 64));
            e0 = (float)(1.001 * (sparse_eps(SIDE) + rho));
            inv_lvl = (float)(1.0 / lvl);
            sparse = la.mode == OFDM_LINK_SCREEN_FORCED || !noise ||
                     sparse_mu<LOGN, FB>(lvl, sigma_d, sc.delta, rho) < kSparseMaxPerQuad;
        }
    }

    const int64_t niter = (cm.n_sym + G::SPB - 1) / G::SPB;
    unsigned long long be = 0, se = 0;
    [[maybe_unused]] unsigned long long screened = 0, redone = 0;  // (lane 0 of each wave counts)
    for (int64_t it = blockIdx.x; it < niter; it += gridDim.x) {
        const int64_t sl = it * G::SPB + ls;
        const int64_t sg = cm.sym0 + sl;
        const bool active = sl < cm.n_sym;
        [[maybe_unused]] bool redo = true;
        if constexpr (SCREEN) {
            if (screen) {
                redo = false;
                if (active) {
                    // the symbol in float32: the complex64 kernels' statements through the same row
                    CF* const rowf = (CF*)row;
                    TxBits<FB, TPS> tb;
                    tb.load(cm, sg, t, nullptr, true);
                    CF xf[E];
                    f32x2 acc = f32x2{0.f, 0.f};
                    using Add = AddPoint<E, TxBits<FB, TPS>>;
                    if constexpr (SCREEN == kLinkScreenTwo) {
                        static_for<0, E>([&](auto I) { xf[I] = lut32[tb.template fixed<I>()]; });
                        fft_sym<float, LOGN, true, FB>(xf, rowf, tt32, tt32 + TTS, t);
                        sym_sync<TPS>();  // the IFFT's last pass has read the row
                        if (noise) {
#pragma unroll
                            for (int i = 0; i < E; ++i) tb.g.add_noise(xf[i].v, ntab, i);
                        }
                        fft_sym<float, LOGN, false, FB>(xf, rowf, tt32, tt32, t);
                        // delta of this symbol, in levels, from its own norm
#pragma unroll
                        for (int i = 0; i < E; ++i) acc = __builtin_elementwise_fma(xf[i].v, xf[i].v, acc);
                    } else {
                        // the noise alone (each sample the once-rounded float32 product), its transform
                        // and that transform's norm; then the point N l32 of each element's subcarrier
#pragma unroll
                        for (int i = 0; i < E; ++i) xf[i] = mk<float>(0.f, 0.f);
                        if (noise) {
                            if constexpr (SPARSE) {
                                ScreenMwc g(tb.g);
#pragma unroll
                                for (int i = 0; i < E; ++i) g.add_noise(xf[i].v, ntab, i);
                            } else {
#pragma unroll
                                for (int i = 0; i < E; ++i) tb.g.add_noise(xf[i].v, ntab, i);
                            }
                            fft_sym<float, LOGN, false, FB>(xf, rowf, tt32, tt32, t);
#pragma unroll
                            for (int i = 0; i < E; ++i) acc = __builtin_elementwise_fma(xf[i].v, xf[i].v, acc);
                        }
                        // (kLinkScreenSparse on its tested path adds the point to the quads it slices, below;
                        // OFDM_ABLATE_RX & 8, ablation builds only: neither the add nor the slicer -- a
                        // timing build, its counts are wrong)
#if OFDM_ABLATION
                        if (!(a.flags & 8))
#endif
                        if (!SPARSE || !sparse) static_for<0, E>(Add{xf, lut32, tb});
                    }
                    const float n2 = wave_sum_f32(acc.x + acc.y);
                    // (a delta of 1/2 or more, or a norm that is not finite: nothing is decisive)
                    const float delta = __builtin_fmaf(cz, __builtin_amdgcn_sqrtf(n2), c0);  // (v_sqrt_f32: 1 ulp)
                    const float thr = delta < 0.5f ? 0.5f - delta : -1.0f;
                    uint32_t bes = 0, ses = 0;
                    float m = 0.f;
                    // quad Q of every lane sliced: its difference word counted, its margin into m
                    const auto slice = [&](auto Q) {
                        constexpr int q = Q;
                        CF z[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = xf[4 * q + j];
                        const uint32_t d = fslicer.template diff_margin<SPARSE>(z, lane_word(tb.lane, q), m);
                        bes += __popc(d);
                        ses += PermSlicer<FB>::nonzero_bytes(d);
                    };
                    if constexpr (SPARSE) {
                        if (sparse) {
                            // a quad no component of which exceeds T, in any lane: d = 0 and m_quad <= thr, proven
                            // (sparse_eps); thr < 0 (delta >= 1/2 or not finite) leaves T < 0: every quad sliced
                            const float T = (thr - e0) * inv_lvl;
                            static_for<0, E / 4>([&](auto Q) {
                                constexpr int q = Q;
                                // (a component that is not finite may drop out of mx, but it has made n2 not
                                // finite, thr = -1 and T < 0 <= mx: every quad is sliced, as before)
                                float mx = max_abs2(xf[4 * q].v);
#pragma unroll
                                for (int j = 1; j < 4; ++j) mx = max_abs3(xf[4 * q + j].v, mx);
                                if (__ballot(!(mx <= T)) != 0) {  // (wave-uniform)
                                    static_for<4 * q, 4 * q + 4>(Add{xf, lut32, tb});
                                    slice(Q);
                                    ++quads.sliced;
                                }
                            });
                            quads.tested += E / 4;
                        }
                    }
                    // (the test stays outside the quad loop: four uniform branches on `sparse` inside it cost the
                    // untested path 2 to 4 %, profiles/link_refactor_ab.txt)
#if OFDM_ABLATION
                    if (!(a.flags & 8))
#endif
                    if (!SPARSE || !sparse) static_for<0, E / 4>(slice);
                    redo = __ballot(!(m <= thr)) != 0;  // one undecided axis: the wave redoes the symbol
                    if constexpr (NOREDO) {  // (counted as redone, taken from its float32 words)
                        be += redo ? bes : 0u;
                        se += redo ? ses : 0u;
                    }
                    if (!redo) {
                        be += bes;
                        se += ses;
                    }
                    if (t == 0) {
                        ++screened;
                        redone += redo;
                    }
                    sym_sync<TPS>();  // the row is rewritten by the redo or the next symbol
                }
            }
        }
        if ((!SCREEN || redo) && !NOREDO) {
            // the lane block: bits for both halves, the generator continuing into the lane's noise
            TxBits<FB, TPS> tb;
            tb.load(cm, sg, t, nullptr, active);
            // transmitter: map and IFFT; x leaves the IFFT as the channel output y
            C x[E];
            static_for<0, E>([&](auto I) { x[I] = lut_s[tb.template fixed<I>()]; });
            fft_sym<R, LOGN, true, FB>(x, row, tt, tt + TTS, t);
            sym_sync<TPS>();  // the IFFT's last pass has read the row
            // receiver: y + AWGN, FFT, slice, compare, count
            if (active && noise) {
#pragma unroll
                for (int i = 0; i < E; ++i) tb.g.add_noise64(x[i].re, x[i].im, ntab64, i);
            }
            fft_sym<R, LOGN, false, FB>(x, row, tt, tt, t);
            if (active) {
                uint32_t bes = 0, ses = 0;
                static_for<0, E / 4>([&](auto Q) {
                    constexpr int q = Q;
                    C z[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = x[4 * q + j];
                    const uint32_t d = pslicer.diff(z, lane_word(tb.lane, q));
                    bes += __popc(d);
                    ses += PermSlicer<FB>::nonzero_bytes(d);
                });
                be += bes;
                se += ses;
            }
            sym_sync<TPS>();  // the FFT row is rewritten by the next symbol
        }
    }
    be = block_sum<unsigned long long, BLK>(be, redc);
    se = block_sum<unsigned long long, BLK>(se, redc);
    if (threadIdx.x == 0) {
        if (be) atomicAdd((unsigned long long*)&a.counters[0], be);
        if (se) atomicAdd((unsigned long long*)&a.counters[1], se);
    }
    if constexpr (SCREEN) {
        if (la.screen_counts) {  // (launch-uniform)
            screened = block_sum<unsigned long long, BLK>(screened, redc);
            redone = block_sum<unsigned long long, BLK>(redone, redc);
            if (threadIdx.x == 0) {
                if (screened) atomicAdd(&la.screen_counts[0], screened);
                if (redone) atomicAdd(&la.screen_counts[1], redone);
            }
            if constexpr (SPARSE) {  // uint64[4]: quads tested, quads sliced behind the screen's two
                const unsigned long long qt = block_sum<unsigned long long, BLK>(t == 0 ? quads.tested : 0u, redc);
                const unsigned long long qs = block_sum<unsigned long long, BLK>(t == 0 ? quads.sliced : 0u, redc);
                if (threadIdx.x == 0) {
                    if (qt) atomicAdd(&la.screen_counts[2], qt);
                    if (qs) atomicAdd(&la.screen_counts[3], qs);
                }
            }
        }
    }
}

// What has a fused form (the one definition: launch_link answers kNoFusedForm for anything
// else and ofdm_link names the reason): a complex128 fixed-QAM bench shape (ref_fb > 1) at a symbol per
// wave with its per-pass twiddles in LDS, a flat channel, no equaliser, Philox streams.
template <typename R, int LOGN>
constexpr int link_fb() {
    if constexpr (sizeof(R) == 8 && ref_fb<R, LOGN>() > 1 && Geo<LOGN>::TPS == 64) {
        if (uses_tt<R, LOGN, ref_fb<R, LOGN>()>()) return ref_fb<R, LOGN>();
    }
    return 0;
}
template <typename R, int LOGN>
static bool link_shape(const LinkArgs& a, int L) {
    if constexpr (link_fb<R, LOGN>() == 0) return false;
    else
        return bench_fixed_shape<link_fb<R, LOGN>()>(a.r.c) && L == 1 && a.r.c.eq == OFDM_EQ_NONE &&
               philox_streams(a.r) && a.r.wide == nullptr;
}

template <typename R, int LOGN>
static hipError_t link_one(const LinkArgs& a, int L, int screen, hipStream_t s) {
    if constexpr (link_fb<R, LOGN>() > 0) {
        if (!link_shape<R, LOGN>(a, L)) return kNoFusedForm;
        constexpr int FB = link_fb<R, LOGN>();
        constexpr int BLK = OFDM_LINK_BLOCK;
        static_assert(Geo<LOGN, BLK>::SPB * Geo<LOGN, BLK>::TPS == BLK, "whole symbols per workgroup");
        // one workgroup holds a CU: two rounds of the resident workgroups, as the receiver it replaces
        const auto go = [&](auto screened) {
            constexpr int SCREEN = decltype(screened)::value;
            CarveSize lds;
            link_carve<R, LOGN, SCREEN, FB>(lds);
            if (lds.bytes + link_static_lds<R, FB>() > kLdsPerCu) return kLdsOverflow;
            return rx_go<BLK, Geo<LOGN, BLK>::SPB>(k_link<R, LOGN, FB, SCREEN>, lds.bytes,
                                                   rx_grid_rounds<R, FB, LOGN>(), a.r.c.n_sym, a, s);
        };
        // screen off: the unscreened kernel itself, not the screened one with its decision forced
        switch (a.mode == OFDM_LINK_SCREEN_OFF ? kLinkScreenNone : screen) {
            case kLinkScreenNone: return go(std::integral_constant<int, kLinkScreenNone>{});
            case kLinkScreenSparse: return go(std::integral_constant<int, kLinkScreenSparse>{});
            case kLinkScreenNoise: return go(std::integral_constant<int, kLinkScreenNoise>{});
            default: return go(std::integral_constant<int, kLinkScreenTwo>{});
        }
    } else {
        return kNoFusedForm;
    }
}

// kNoFusedForm: no fused form for this plan or these arguments (nothing launched)
template <typename R>
hipError_t launch_link(int logn, int L, const LinkArgs& a, int screen, hipStream_t s) {
    return with_logn(logn, [&](auto l) { return link_one<R, decltype(l)::value>(a, L, screen, s); });
}

}  // namespace ofdm
