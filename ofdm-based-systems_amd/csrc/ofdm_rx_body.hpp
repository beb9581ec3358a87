// ofdm_rx_body.hpp -- the body of the fused receivers k_rx and k_rx_prof (ofdm_fused.hpp), included
// into each kernel after its `constexpr bool PROF` (no include guard: included once per kernel).
// In scope: the kernel's template parameters R, LOGN, EQ, FB, MV, REF, WIDE, its argument `RxArgs a`,
// the form's facts FORM (RxFormOf: its ONE_WAVE is the workgroup shape) and PROF, SWEEP, FRAMES and DENS.
// DENS (k_rx_dens only, which defines OFDM_RX_BODY_DENS around its include and has its second argument
// `RxDensTail dt` in scope): every equalised point is also binned into the density histogram in LDS.
// FRAMES (k_rx_frames only, which defines OFDM_RX_BODY_FRAMES around its include and has its second
// argument `RxFramesTail ft` in scope): each symbol's counts are also added to its frame's pair.
// FRAMES and SWEEP (k_rx_sweep_frames only, which defines both macros and has `sa` and `ft` in scope): the
// frame block runs inside the point loop, where bes / ses are the symbol's at the point, and adds them
// to the point's rows of a point-major record, frames[pt][frame][2].
// SOFT (k_rx_soft only, which defines OFDM_RX_BODY_SOFT around its include and has its second argument
// `RxSoftTail st` in scope; FORM::SOFT): every compared bit of every element in range is also binned into
// the soft-decision histogram in LDS, at the three places where DENS takes its point.
// SWEEP (k_rx_sweep only, which defines OFDM_RX_BODY_SWEEP around its include and has its argument
// `RxSweepArgs sa` in scope, `a` being sa.r): every symbol is received once per SNR
// point, the point loop opened and closed under that macro so that the other kernels' text has no loop.
    static_assert(!WIDE || (FB == 0 && EQ == -1 && !REF), "the wide slicer lives in the generic kernel");
    static_assert(!PROF || (!REF && (FB == 0 || (sizeof(R) == 8 && (FB == 1 || !(FB & 1)) && (FB == 1 || !MV)))),
                  "the profile: the generic kernel, or a complex128 cyclic-prefix OFDM QAM throughput receiver");
    static_assert(!SWEEP || (!REF && !WIDE && !PROF && (FB == 0 || (sizeof(R) == 8 && FB > 1 && !(FB & 1) && !MV))),
                  "the sweep: the generic kernel, or a complex128 cyclic-prefix OFDM fixed-QAM throughput receiver");
#if defined(OFDM_RX_BODY_FRAMES) && defined(OFDM_RX_BODY_SWEEP)
    // (k_rx_sweep_frames, the one kernel with both: the sweep's own condition above holds for it)
    static_assert(FRAMES && SWEEP, "the frame record of a sweep: k_rx_sweep_frames defines both macros around its include");
#define OFDM_RX_FRAME_ROW(f) ((int64_t)pt * ft.n_frames + (f))  // point-major: the point's rows
#elif defined(OFDM_RX_BODY_FRAMES)
    static_assert(FRAMES && !REF && !PROF && !SWEEP &&
                      (FB == 0 || (sizeof(R) == 8 && (FB == 1 || !(FB & 1)) && (FB == 1 || !MV))),
                  "the frame record: the generic kernel, or a complex128 cyclic-prefix OFDM QAM throughput receiver");
#define OFDM_RX_FRAME_ROW(f) (f)
#else
    static_assert(!FRAMES, "k_rx_frames defines OFDM_RX_BODY_FRAMES around its include");
#endif
#ifdef OFDM_RX_BODY_DENS
    static_assert(DENS && !REF && !PROF && !SWEEP && !FRAMES &&
                      (FB == 0 || (sizeof(R) == 8 && (FB == 1 || !(FB & 1)) && (FB == 1 || !MV))),
                  "the density record: the generic kernel, or a complex128 cyclic-prefix OFDM QAM throughput receiver");
#else
    static_assert(!DENS, "k_rx_dens defines OFDM_RX_BODY_DENS around its include");
#endif
#ifdef OFDM_RX_BODY_SOFT
    static_assert(FORM::SOFT && !REF && !WIDE && !PROF && !SWEEP && !FRAMES && !DENS &&
                      (FB == 0 || (sizeof(R) == 8 && (FB == 1 || !(FB & 1)) && (FB == 1 || !MV))),
                  "the soft record: the generic kernel, or a complex128 cyclic-prefix OFDM QAM throughput receiver");
#else
    static_assert(!FORM::SOFT, "k_rx_soft defines OFDM_RX_BODY_SOFT around its include");
#endif
#ifdef OFDM_RX_BODY_SWEEP
#define OFDM_RX_SNR_LIN snr_lin_pt  // the SNR of the point being received
#else
#define OFDM_RX_SNR_LIN a.snr_lin
#endif
    constexpr int BLK = rx_block<R, FB, LOGN, EQ, MV, FORM::ONE_WAVE>();
    using G = Geo<LOGN, BLK>;
    using C = cpx<R>;
    constexpr int N = G::N, E = G::E, TPS = G::TPS;
    const TxRxCommon& cm = a.c;
    const int flags = ablation_flags(a.flags);
    const int eq = EQ >= 0 ? EQ : cm.eq;
    const bool adaptive = FB ? false : (bool)cm.adaptive;
    // generic kernel variants: single-carrier OFDM (FFT -> equalise -> IFFT,
    // modulation/models.py:72-91), zero-padding guard (overlap-add, prefix/models.py:69-101)
    // and non-separable constellations (PSK: brute-force nearest point, constellation/models.py:19-27)
    constexpr bool F64_FAST = sizeof(R) == 8 && FB > 0;  // complex128 throughput kernels
    const bool scm = (FB == 1 || !MV) ? false : (bool)cm.scm;  // SC-OFDM (run-time, uniform)
    const bool zp = (FB == 1 || !MV) ? false : (bool)cm.zpad;  // zero-padding guard (run-time, uniform)
    const bool nn = FB ? false : (bool)cm.nn;
    const int ystride = (FB == 1 || !MV) ? N : cm.ystride;
    // odd bits per subcarrier (FB = 3, 5): the reference's 8- / 32-PSK only
    constexpr bool FB_PSK_ONLY = FB > 1 && (FB & 1);
    // noise phase table: static LDS at a link-time constant address, so a sample's entry offset
    // (from its phase word) addresses it with no add
    __shared__ f32x2 ntab[kNoisePhases];
    // complex128 throughput kernels: the table widened to double (Mwc64x::add_noise64)
    __shared__ f64x2 ntab64_s[rx_ntab64_static<R, FB>()];
    f64x2* ntab64 = F64_FAST ? ntab64_s : nullptr;
    Carve cv(ofdm_smem);
    constexpr bool TT = uses_tt<R, LOGN, FB>();
    constexpr bool SPLIT = split_rows<R, FB>();  // complex128 throughput: rows of reals
    constexpr int TTS = TT ? tt_size(LOGN) : 0;
    const int tts_all = rx_tts<R, LOGN, FB>(scm);
    // a plan with an order above 256 (WIDE): the wide slicer's level patterns in LDS
    const int n_wide = WIDE ? cm.n_axis : 0;
    // SWEEP: the per-point noise tables and counters (the throughput form keeps y and the noise radii
    // in registers across the points, HOLD; the generic one reloads y and replays the generator)
#ifdef OFDM_RX_BODY_SWEEP
    const int n_sweep = sa.n_snr;
#else
    constexpr int n_sweep = 0;
#endif
    constexpr bool HOLD = SWEEP && F64_FAST;
    const RxLds<R> lds = rx_carve<R, LOGN, EQ, FB, MV, FORM::ONE_WAVE>(cv, cm.words_per_sym, tts_all, n_wide, n_sweep);
    C *tw = lds.tw, *tt = lds.tt, *eqt = lds.eqt;
    AxisInfo* axis = lds.axis;
    unsigned char* rowmem = lds.rowmem;
    uint32_t* words = lds.words;
    R* red = lds.red;
    unsigned long long* redc = lds.redc;
    using OP = typename RxLds<R>::OP;
    OP* ordt = lds.ordt;
#ifdef OFDM_RX_BODY_DENS
    // DENS: the workgroup's histogram behind the receiver's layout, zeroed before the first barrier
    uint32_t* const dhist = dens_lds(cv, dt.bins);
    const int dcells = dt.bins * dt.bins;
    for (int i = threadIdx.x; i < dcells; i += BLK) dhist[i] = 0;
    unsigned long long dout = 0;  // the lane's points outside the square
    uint32_t dleft = dt.flush;    // iterations until the bins must be flushed (RxDensTail)
    // the workgroup's bins into the record: one 64-bit integer atomic per non-empty bin (between barriers)
    auto dens_flush = [&](bool zero) {
        for (int i = threadIdx.x; i < dcells; i += BLK) {
            const uint32_t c = dhist[i];
            if (c) {
                atomicAdd(dt.hist + i, (unsigned long long)c);
                if (zero) dhist[i] = 0;
            }
        }
    };
#endif
#ifdef OFDM_RX_BODY_SOFT
    // SOFT: the plan's level table and the workgroup's histogram behind the receiver's layout, the table
    // staged and the bins zeroed before the first barrier
    const SoftLds sl_ = soft_lds(cv, st.bins);
    uint32_t* const shist = sl_.hist;
    const int scells = kSoftRows * 2 * st.bins;
    for (int i = threadIdx.x; i < scells; i += BLK) shist[i] = 0;
    for (int i = threadIdx.x; i < cm.n_axis * 2 * kSoftSide; i += BLK) sl_.lev[i] = st.lev[i];
    unsigned long long sinv = 0;  // the lane's NaN bits
    uint32_t sleft = st.flush;    // iterations until the bins must be flushed (RxSoftTail)
    // the workgroup's bins into the record: one 64-bit integer atomic per non-empty bin (between barriers)
    auto soft_flush = [&](bool zero) {
        for (int i = threadIdx.x; i < scells; i += BLK) {
            const uint32_t c = shist[i];
            if (c) {
                atomicAdd(st.hist + i, (unsigned long long)c);
                if (zero) shist[i] = 0;
            }
        }
    };
#endif
    constexpr bool EQ_LDS = eq_in_lds<R, FB, LOGN, EQ>();  // (rx_carve)
    // otherwise (throughput kernels at N = 4096, and the complex64 generic kernel) the lane's
    // coefficients are loaded before the FFT each symbol (L2-resident), so their latency hides
    // behind it instead of stalling each element of the equaliser
    constexpr bool EQ_LATE = rx_eq_late<R, FB, LOGN, EQ>();
    constexpr bool EQ_PRE =
        !EQ_LDS && !EQ_LATE && ((FB > 0 && EQ > OFDM_EQ_NONE) || (FB == 0 && sizeof(R) == 4));
    constexpr bool EQ_REG = EQ_PRE || EQ_LATE;  // coefficients in registers (ecoef)
    constexpr bool MMSE_BATCH = sizeof(R) == 8 && FB > 0 && EQ == OFDM_EQ_MMSE;

    // the tables' global reads issued first (Staged), the noise table built while they fly
    Staged<BLK, (FB > 1 && MV ? 2 : 1) * TTS, C> st_tt;
    Staged<BLK, EQ_LDS ? N : 0, C> st_eq;
    Staged<BLK, kMaxLuts, Dwords<AxisInfo>> st_ax;
    static_assert(kMaxLuts <= BLK, "one axis entry per thread");
    st_tt.load((const C*)cm.ptw, tts_all);
    if constexpr (EQ_LDS) st_eq.load((const C*)cm.eq_a, N);
    st_ax.load((const Dwords<AxisInfo>*)cm.axis, cm.n_axis);
    // sigma from the whole-stream mean power (noise/models.py:13-22)
    const bool noise = a.noise_on && !(flags & 1);
    double sigma_d = 0;
    if (noise) {
        const double p = a.stats[0] / (double)a.total_samples;
        sigma_d = sqrt((p / a.snr_lin) / 2.0);
    }
    const R sigma = (R)sigma_d;
    build_noise_table(ntab, sigma_d, ntab64);
#ifdef OFDM_RX_BODY_SWEEP
    // one phase table per point, each entry as build_noise_table makes it from the point's sigma (the
    // single table above is not read), and the workgroup's per-point counts zeroed
    {
        const double pw = a.stats[0] / (double)a.total_samples;
        for (int i = threadIdx.x; i < n_sweep * kNoisePhases; i += BLK) {
            const f32x2 e = noise_table_entry(sqrt((pw / sa.snr_lin[i / kNoisePhases]) / 2.0), i % kNoisePhases);
            if constexpr (HOLD)
                lds.sntab64[i] = f64x2{(double)e.x, (double)e.y};
            else
                lds.sntab[i] = e;
        }
        for (int i = threadIdx.x; i < 2 * n_sweep; i += BLK) lds.scnt[i] = 0;
    }
#endif
    if constexpr (!TT) load_twiddles<R>(tw, (const C*)cm.tw);
    st_tt.store(tt);
    if constexpr (EQ_LDS) st_eq.store(eqt);
    st_ax.store((Dwords<AxisInfo>*)axis);
    // PROF, throughput receivers: the LUT pool staged for the transmitted points
    [[maybe_unused]] C* plut = nullptr;
    if constexpr (PROF && FB > 0) {
        plut = prof_lut<C, FB>();
        for (int i = threadIdx.x; i < cm.lut_len && i < prof_lut_static<FB>(); i += BLK) plut[i] = ((const C*)cm.lut)[i];
    }
    if constexpr (WIDE) {
        for (int i = threadIdx.x; i < n_wide * kWideSide; i += BLK) {
            const int l = i / kWideSide, k = i % kWideSide;
            lds.wpat[2 * kWideSide * l + k] = a.wide[l].ipat[k];
            lds.wpat[2 * kWideSide * l + kWideSide + k] = a.wide[l].qpat[k];
        }
    }
    if constexpr (FB == 1 && sizeof(R) == 8) {
        if (threadIdx.x < 8) {
            OrderParams64 o = OrderParams64::make(0.0, 0.0, 0.0, 0u);  // unused subcarrier: level 0, no bits
            if (threadIdx.x < cm.n_axis && threadIdx.x != kUnusedOrder) {
                const AxisInfo ax = __builtin_bit_cast(AxisInfo, st_ax.v[0]);  // (thread < n_axis <= kMaxLuts)
                const double span = (double)(ax.side - 1);
                o = OrderParams64::make(ax.inv_step * cm.scale / span,  // mul: the FFT output stays unscaled
                                        ax.lev0 * ax.inv_step / span,   // add: negated in the FMA
                                        span, ((1u << ax.bits) - 1u) | ((1u << ax.hbits) << 8));
            }
            ordt[threadIdx.x] = o;
        }
    } else if constexpr (FB == 1) {
        if (threadIdx.x < 8) {
            // unused subcarrier: level 0, no bits
            OrderParams o{0.f, 0.f, 0u, 0u};
            if (threadIdx.x < cm.n_axis && threadIdx.x != kUnusedOrder) {
                const AxisInfo ax = __builtin_bit_cast(AxisInfo, st_ax.v[0]);  // (thread < n_axis <= kMaxLuts)
                const double span = (double)(ax.side - 1);  // see OrderParams
                o.mul = (float)(ax.inv_step * cm.scale / span);  // the FFT output stays unscaled
                o.add = (float)(-ax.lev0 * ax.inv_step / span);
                o.smax = __float_as_uint((float)(ax.side - 1));
                o.meta = ((1u << ax.bits) - 1u) | ((1u << ax.hbits) << 8);
            }
            ordt[threadIdx.x] = o;
        }
    }
    __syncthreads();

    // a symbol group of >= 64 threads is whole wavefronts: make its index wave-uniform
    const int ls = TPS >= 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x / TPS) : threadIdx.x / TPS;
    const int t = threadIdx.x % TPS;
    C* row = (C*)(rowmem + (size_t)ls * G::PADN * (SPLIT ? sizeof(R) : sizeof(C)));
    uint32_t* W = words + ls * cm.words_per_sym;
    const C* eqa = (const C*)cm.eq_a;
    const __amdgpu_buffer_rsrc_t eq_rsrc = buf_rsrc(eqa, (uint32_t)(N * sizeof(C)));
    const R* eqb = (const R*)cm.eq_b;
    // ZF / MMSE of subcarrier k (equalization/models.py:22-63); nv: the symbol's MMSE noise variance
    // (pa: the coefficient the throughput kernel preloaded for this element, or null)
    auto eq_apply = [&](C v, int k, R nv, const C* pa) -> C {
        if constexpr (EQ_LDS || EQ_REG) {
            // ZF 1/H; MMSE conj(H) with |H|^2 recomputed from it (complex64 only)
            const C c = EQ_LDS ? eqt[k] : *pa;
            if (eq == OFDM_EQ_ZF) return cmul(v, c);
            const R d = c.re * c.re + c.im * c.im + nv;  // |H|^2 + nv
            return cscale(cmul(v, c), recip<R>(d));
        } else {
            if (eq == OFDM_EQ_ZF) return cmul(v, eqa[k]);
            if (eq == OFDM_EQ_MMSE) return cmul(v, mmse_coef<R>(eqa[k], eqb[k], nv));
            return v;
        }
    };
    const int cp = cm.cp;
    const R scale = (R)cm.scale;
    Slicer<R> slicer;
    std::conditional_t<sizeof(R) == 8, PermSlicer64<(FB > 1 ? FB : 2)>, PermSlicer<(FB > 1 ? FB : 2)>> pslicer;
    // adaptive throughput kernel: the LDS byte offset of each element's order entry, four
    // elements per word (the lane's subcarriers do not change from symbol to symbol)
    uint32_t ocode[FB == 1 ? E / 4 : 1];
    bool small_orders = false;  // adaptive: every order <= 64 (3-bit levels)
    const double magic64 = PermSlicer64<2>::uniform(6755399441055744.0);  // 1.5 * 2^52 (complex128)
    if constexpr (FB == 1) {
        int side = 0;
        for (int l = 0; l < cm.n_axis; ++l) side = max(side, (int)axis[l].side);
        small_orders = side <= 8;
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int lid = cm.sc[t + (4 * q + j) * TPS].lut;
                w |= (uint32_t)(sizeof(OP) * (lid < 0 ? kUnusedOrder : lid)) << (8 * j);
            }
            ocode[q] = w;
        }
    } else if constexpr (FB > 1 && !FB_PSK_ONLY) {
        // the FFT output stays unscaled (x sqrt N); SC-OFDM adds the unscaled IFFT (x sqrt N).
        // The reference's 4/16-PSK (psk_m > 0) decide by sector and have no axis tables.
        if (cm.psk_m == 0) pslicer.load(axis[0], scm ? cm.scale * cm.scale : cm.scale);
    } else if (!adaptive) {
        // (its nibble patterns hold sides <= 16; a wide plan decides by slice_wide)
        if constexpr (!WIDE) slicer.load(axis[0]);
    }

    const bool array_noise = (FB == 0 || REF) && a.nr != nullptr && noise;
    const int64_t niter = (cm.n_sym + G::SPB - 1) / G::SPB;
    unsigned long long be = 0, se = 0;
    // PROF: element i's bit errors, symbol errors and clipped samples, and the two fixed-point
    // limbs of its error-vector power (fx_accum), over the symbols this lane processes
    constexpr int PE = PROF ? E : 1;
    uint32_t pbe[PE] = {}, pse[PE] = {}, pcl[PE] = {};
    unsigned long long pl0[PE] = {}, pl1[PE] = {};

    // kept channel samples of local symbol sl.  Past the end the wave reads the last symbol
    // again (its results are neither counted nor stored): an unconditional load, where zeroing
    // the 16 elements cost 32 v_mov_b64 per symbol in complex128.  Zeros when ablated.
    // (symbols of 2 / 4 waves too, N = 2048 / 4096: the row base is wave-uniform when TPS >= 64;
    // RX d 4.67 -> 4.63, e 4.15 -> 4.12 ms per step, profiles/r04h_ab_rxbuf_ch64.txt)
    constexpr bool RX_BUF = F64_FAST && TPS >= 64;
    auto load_sym = [&](int64_t sl, C (&dst)[E]) {
        const C* ys = (const C*)a.y + (sl < cm.n_sym ? sl : cm.n_sym - 1) * ystride;
        if (RX_BUF && !(flags & 16)) {
            // complex128, a symbol per wave: buffer loads off the symbol's row, the lane's byte
            // offset in one VGPR and element i's in the instruction's SGPR offset
            if constexpr (RX_BUF) {
                const __amdgpu_buffer_rsrc_t r = buf_rsrc(ys, (uint32_t)(N * sizeof(C)));
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    dst[i] = buf_load16<C, (bool)OFDM_RX_NT>(r, (uint32_t)t * (uint32_t)sizeof(C),
                                                             (uint32_t)(i * TPS * (int)sizeof(C)));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else if (!(flags & 16)) {
            // issued in element order, the order the noise consumes them: each add then waits
            // for its own load only (left to the scheduler, the N = 4096 complex128 RX issued
            // element 0 thirteenth and waited for 13 of 16 loads before its first add)
#pragma unroll
            for (int i = 0; i < E; ++i) {
                dst[i] = ld_stream<(FB > 0 && OFDM_RX_NT)>(ys + t + i * TPS);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) dst[i] = mk<R>(0, 0);
        }
    };
    for (int64_t it = blockIdx.x; it < niter; it += gridDim.x) {
        const int64_t sl = it * G::SPB + ls;
        const int64_t sg = cm.sym0 + sl;
        const bool active = sl < cm.n_sym;
        TxBits<FB, TPS, REF> tb;
        // kept channel samples + AWGN; the 1/sqrt(N) of fft(norm="ortho") folded in
        const C* ys = (const C*)a.y + sl * ystride;
        C x[E];
        tb.load(cm, sg, t, W, active && (!(flags & 4) || (noise && !array_noise)));
#ifdef OFDM_RX_BODY_SWEEP
        // What does not depend on the SNR, once per symbol: the lane block (above) and, HOLD, the kept
        // samples and the lane's noise words -- the 16 float32 radii and the four phase words stay in
        // registers across the points.  The generic form keeps the generator's state instead and, per
        // point, reloads y (cached) and draws the same words again: zero padding's tail samples too.
        [[maybe_unused]] C y0[HOLD ? E : 1];
        [[maybe_unused]] float rad[HOLD ? E : 1] = {};
        [[maybe_unused]] uint32_t qw[HOLD ? E / 4 : 1] = {};
        const uint32_t g0x = tb.g.x, g0c = tb.g.c;
        if constexpr (HOLD) {
            load_sym(sl, y0);
            if (active && noise) {
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const uint32_t w = tb.g.draw(i);
                    if ((i & 3) == 0) qw[i >> 2] = tb.g.q;
                    rad[i] = noise_radius(w);
                }
            }
        }
        for (int pt = 0; pt < n_sweep; ++pt) {
        const double snr_lin_pt = sa.snr_lin[pt];  // (the MMSE noise variance's: OFDM_RX_SNR_LIN)
        // the point's phase table under the single-point table's name: the noise code below is k_rx's
        [[maybe_unused]] const f32x2* const ntab = lds.sntab + pt * kNoisePhases;
        if constexpr (HOLD) {
            // x = y + noise_k as add_noise64 forms it, from the held radius and phase words
            const f64x2* const tab64 = lds.sntab64 + pt * kNoisePhases;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const uint32_t off = ((qw[i >> 2] >> (8 * (i & 3))) & (uint32_t)(kNoisePhases - 1)) * (uint32_t)sizeof(f64x2);
                const f64x2 e = *(const f64x2*)((const unsigned char*)tab64 + off);
                const double rd = (double)rad[i];
                x[i].re = __builtin_fma(rd, e.x, y0[i].re);
                x[i].im = __builtin_fma(rd, e.y, y0[i].im);
            }
        } else {
            tb.g.x = g0x;
            tb.g.c = g0c;
        }
#endif
        if constexpr (!HOLD) load_sym(sl, x);
        if (active && array_noise) {
            const double* nr = a.nr + sg * (N + cp) + (zp ? 0 : cp);
            const double* ni = a.ni + sg * (N + cp) + (zp ? 0 : cp);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                x[i].re += sigma * (R)nr[t + i * TPS];
                x[i].im += sigma * (R)ni[t + i * TPS];
            }
        } else if (active && noise && !HOLD) {
            // noise sample j = i of the lane: a radius word per element, a phase word per four
            // (stream version 3, ofdm_device.hpp "throughput-mode streams")
#pragma unroll
            for (int i = 0; i < E; ++i) {
                if constexpr (sizeof(R) == 4) {
                    tb.g.add_noise(x[i].v, ntab, i);
                } else if constexpr (F64_FAST) {
                    tb.g.add_noise64(x[i].re, x[i].im, ntab64, i);
                } else {
                    tb.g.add_noise_f64(x[i].re, x[i].im, ntab, i);
                }
            }
        }
        if (zp && active) {
            // zero guard: received sample N + k (k < cp) is added onto sample k, noise included
            // (philox mode: the lane's noise samples continue, tail sample i is sample E + i -- the
            // tail samples a lane owns are its first ones, k < cp)
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int k = t + i * TPS;
                if (k < cp) {
                    C v = (flags & 16) ? mk<R>(0, 0) : ys[N + k];
                    if (array_noise) {
                        v.re += sigma * (R)a.nr[sg * (N + cp) + N + k];
                        v.im += sigma * (R)a.ni[sg * (N + cp) + N + k];
                    } else if (noise) {
                        if constexpr (sizeof(R) == 8) {
                            tb.g.add_noise_f64(v.re, v.im, ntab, E + i);
                        } else {
                            const f32x2 n = tb.g.noise(ntab, E + i);
                            v = v + mk<R>(n.x, n.y);
                        }
                    }
                    x[i] = x[i] + v;
                }
            }
        }
        if constexpr (FB == 0) {
#pragma unroll
            for (int i = 0; i < E; ++i) x[i] = cscale(x[i], scale);
        }
        C ecoef[EQ_REG ? E : 1];
        if constexpr (EQ_PRE) {
            if (eq != OFDM_EQ_NONE) {
#pragma unroll
                for (int i = 0; i < E; ++i) ecoef[i] = eqa[t + i * TPS];
            }
        }
        if (!(flags & 2)) fft_sym<R, LOGN, false, FB>(x, row, tw, tt, t);
        // (late loads: the first four here, each later four one slicer group ahead)
        // (buffer loads, the lane's byte offset + element i's in an SGPR: one address VGPR, where
        // 16 hoisted 64-bit addresses spilled at 3 waves per SIMD)
        auto load_coef4 = [&](int q) {
            if constexpr (EQ_LATE) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    ecoef[4 * q + j] = buf_load16<C>(eq_rsrc, (uint32_t)t * (uint32_t)sizeof(C),
                                                     (uint32_t)((4 * q + j) * TPS * (int)sizeof(C)));
            }
        };
        if constexpr (EQ_LATE) load_coef4(0);
        if (FB == 0) sym_sync<TPS>();  // staged words visible to the whole group
        // MMSE noise variance per OFDM symbol (equalization/models.py:39-49)
        R nv = 0;
        if (eq == OFDM_EQ_MMSE) {
            R p = 0;
            if constexpr (sizeof(R) == 4) {
                f32x2 pacc = f32x2{0.f, 0.f};  // (sum Re^2, sum Im^2): one packed FMA per element
#pragma unroll
                for (int i = 0; i < E; ++i) pacc = __builtin_elementwise_fma(x[i].v, x[i].v, pacc);
                p = pacc.x + pacc.y;
            } else {
#pragma unroll
                for (int i = 0; i < E; ++i) p += norm2(x[i]);
            }
            p = group_sum<R, TPS>(p, red);
            if constexpr (FB > 0) p *= scale * scale;  // power of the ortho-scaled spectrum
            nv = cm.gain_mean == 0.0 ? (R)INFINITY : ((p / (R)N) / (R)OFDM_RX_SNR_LIN) / (R)cm.gain_mean;
        }
        if (scm) {
            // single carrier: equalise every subcarrier, back to time with ifft(ortho)
            if constexpr (EQ_LATE) {
                load_coef4(1);
                load_coef4(2);
                load_coef4(3);
            }
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (eq != OFDM_EQ_NONE)
                    x[i] = eq_apply(x[i], t + i * TPS, nv, &ecoef[EQ_REG ? i : 0]);
            sym_sync<TPS>();  // the forward FFT has read the row
            if constexpr (FB > 1) {
                fft_sym<R, LOGN, true, FB>(x, row, tw, tt + TTS, t);  // 1/N in the slicer
            } else {
                fft_reg<R, LOGN, true, false>(x, row, tw, tw + 64, t, tt);
#pragma unroll
                for (int i = 0; i < E; ++i) x[i] = cscale(x[i], scale);
            }
        }
        if (active && !(flags & 8)) {
            const int64_t sbit = sg * cm.bps;
            const bool all_valid = FB > 1 || sbit + cm.bps <= a.n_valid_bits;
            uint32_t bes = 0, ses = 0;
            auto equalized = [&](int i) {
                if (scm || eq == OFDM_EQ_NONE) return x[i];  // single carrier: equalised before the IFFT
                return eq_apply(x[i], t + i * TPS, nv, &ecoef[EQ_REG ? i : 0]);
            };
            // MMSE in complex128: conj(H) v / (|H|^2 + nv) of a lane word's four elements, the four
            // reciprocals from one (MMSE_BATCH)
            // (sc non-null: z = conj(H) v unscaled and sc[j] = 1 / (|H|^2 + nv), the slicer folding the
            // scale into its level multiplier: one product per element instead of two)
            auto mmse4 = [&](int q, C(&z)[4], R* sc) {
                C c[4];
                R dn[4], inv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c[j] = EQ_LDS ? eqt[t + (4 * q + j) * TPS] : ecoef[EQ_REG ? 4 * q + j : 0];
                    dn[j] = c[j].re * c[j].re + c[j].im * c[j].im + nv;
                }
                const R p01 = dn[0] * dn[1], p012 = p01 * dn[2], p = p012 * dn[3];
                if (__builtin_expect(p >= (R)1e-280 && p <= (R)1e280, 1)) {
                    R r = recip<R>(p);  // 1 / (d0 d1 d2 d3)
                    inv[3] = r * p012;
                    r *= dn[3];  // 1 / (d0 d1 d2)
                    inv[2] = r * p01;
                    r *= dn[2];  // 1 / (d0 d1)
                    inv[1] = r * dn[0];
                    inv[0] = r * dn[1];
                } else {  // a zero, infinite or extreme factor: one reciprocal each
#pragma unroll
                    for (int j = 0; j < 4; ++j) inv[j] = recip<R>(dn[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (sc) {
                        z[j] = cmul(x[4 * q + j], c[j]);
                        sc[j] = inv[j];
                    } else {
                        z[j] = cscale(cmul(x[4 * q + j], c[j]), inv[j]);
                    }
                }
            };
            if constexpr (FB == 1) {
                // four elements per lane word, each through its subcarrier's order (the codes
                // are made opaque per symbol: the order-table reads stay inside the loop)
                static_for<0, E / 4>([&](auto Q) {
                    constexpr int q = Q;
                    if constexpr (EQ_LATE && q + 1 < E / 4) load_coef4(q + 1);
                    C z[4];
                    const OP* op[4];
                    uint32_t oc = ocode[q];
                    asm volatile("" : "+v"(oc));
                    R sc[4] = {1, 1, 1, 1};  // the MMSE scale per element, folded into the slicer
                    if (MMSE_BATCH) {
                        mmse4(q, z, sc);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = equalized(4 * q + j);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        op[j] = (const OP*)((const unsigned char*)ordt + ((oc >> (8 * j)) & 0xFFu));
                    uint32_t d;
                    if constexpr (sizeof(R) == 8)
                        d = small_orders ? adaptive_diff64<true, MMSE_BATCH>(z, op, lane_word(tb.lane, q), magic64, sc)
                                         : adaptive_diff64<false, MMSE_BATCH>(z, op, lane_word(tb.lane, q), magic64, sc);
                    else
                        d = small_orders ? adaptive_diff<true>(z, op, lane_word(tb.lane, q))
                                         : adaptive_diff<false>(z, op, lane_word(tb.lane, q));
                    ses += PermSlicer<8>::nonzero_bytes(d);
                    if constexpr (PROF) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) pse[4 * q + j] += ((d >> (8 * j)) & 0xFFu) != 0u;
                    }
                    if (!all_valid) {
                        // a trailing partial byte of the run is not compared (constellation/
                        // adaptive.py:259-263): keep the first bits (MSB first) of the valid range.
                        static_assert(sizeof(ScInfo) == 8, "ScInfo is one 8-byte word");
                        gptr<const uint64_t> scp = (gptr<const uint64_t>)cm.sc;
                        uint32_t vm = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const ScInfo sc = __builtin_bit_cast(ScInfo, (uint64_t)scp[t + (4 * q + j) * TPS]);
                            if (sc.lut < 0) continue;
                            const int64_t nvb = a.n_valid_bits - (sbit + sc.bitoff);
                            const int keep = nvb <= 0 ? 0 : (nvb >= sc.bits ? sc.bits : (int)nvb);
                            vm |= (((1u << keep) - 1u) << (sc.bits - keep)) << (8 * j);
                        }
                        d &= vm;
                    }
                    bes += __popc(d);
#ifdef OFDM_RX_BODY_DENS
                    // DENS: the point k_rx_prof forms for its error vector (an order-0 subcarrier has none)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = t + (4 * q + j) * TPS;
                        if ((int)((oc >> (8 * j)) & 0xFFu) / (int)sizeof(OP) == kUnusedOrder) continue;
                        if (k >= dt.k_lo && k < dt.k_hi) dens_bin<R>(cscale(z[j], sc[j] * scale), dt, dhist, dout);
                    }
#endif
#ifdef OFDM_RX_BODY_SOFT
                    // SOFT: the point k_rx_prof forms, the lane byte's transmitted index and the byte of the
                    // valid-bit mask d was compared under (an order-0 subcarrier carries nothing)
                    {
                        uint32_t vmw = 0xFFFFFFFFu;
                        if (!all_valid) {
                            gptr<const uint64_t> scp = (gptr<const uint64_t>)cm.sc;
                            vmw = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const ScInfo sc = __builtin_bit_cast(ScInfo, (uint64_t)scp[t + (4 * q + j) * TPS]);
                                if (sc.lut < 0) continue;
                                const int64_t nvb = a.n_valid_bits - (sbit + sc.bitoff);
                                const int keep = nvb <= 0 ? 0 : (nvb >= sc.bits ? sc.bits : (int)nvb);
                                vmw |= (((1u << keep) - 1u) << (sc.bits - keep)) << (8 * j);
                            }
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = t + (4 * q + j) * TPS;
                            const int lid = (int)((oc >> (8 * j)) & 0xFFu) / (int)sizeof(OP);
                            if (lid == kUnusedOrder || k < st.k_lo || k >= st.k_hi) continue;
                            const uint32_t ti = (lane_word(tb.lane, q) >> (8 * j)) & ((1u << axis[lid].bits) - 1u);
                            soft_bin<4, R>(cscale(z[j], sc[j] * scale), (int)axis[lid].hbits, ti, (vmw >> (8 * j)) & 0xFFu,
                                           sl_.lev + lid * 2 * kSoftSide, st.g[k], st, shist, sinv);
                        }
                    }
#endif
                    if constexpr (PROF) {
                        // per element: the masked bit count from its byte of d; the error vector from
                        // z times its MMSE scale and the 1/sqrt(N) the slicer folds in, against the
                        // staged LUT point of the lane byte (an unused subcarrier stays zero)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int lid = (int)((oc >> (8 * j)) & 0xFFu) / (int)sizeof(OP);
                            if (lid == kUnusedOrder) continue;
                            pbe[4 * q + j] += __popc((d >> (8 * j)) & 0xFFu);
                            const uint32_t ti = (lane_word(tb.lane, q) >> (8 * j)) & ((1u << axis[lid].bits) - 1u);
                            prof_power<R>(cscale(z[j], sc[j] * scale), plut[axis[lid].lut_off + (int)ti],
                                          pl0[4 * q + j], pl1[4 * q + j], pcl[4 * q + j]);
                        }
                    }
                });
            } else if constexpr (FB > 0) {
                // four elements per lane word: slice, look up, compare, count
                static_for<0, E / 4>([&](auto Q) {
                    constexpr int q = Q;
                    if constexpr (EQ_LATE && q + 1 < E / 4) {
                        if (!scm) load_coef4(q + 1);  // (single carrier: loaded before its equaliser)
                    }
                    C z[4];
                    R sc[4];  // MMSE_BATCH: the scale per element, folded into the QAM slicer
                    const bool fold = MMSE_BATCH && !scm;
                    if (fold) {
                        mmse4(q, z, sc);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[j] = equalized(4 * q + j);
                    }
                    uint32_t d = 0;
                    // the reference's M-PSK (M <= 32: 4- and 16-PSK share the QAM kernels'
                    // FB = 2 / 4, 8- and 32-PSK have FB = 3 / 5 to themselves): sector
                    // decisions (psk_decide); compiled out of the 64/256-QAM kernels
                    if (FB_PSK_ONLY || (FB <= 4 && cm.psk_m > 0)) {
                        uint32_t r = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) r |= psk_decide(fold ? cscale(z[j], sc[j]) : z[j], cm) << (8 * j);
                        d = r ^ (lane_word(tb.lane, q) & PermSlicer<FB>::BYTE_MASK);
                    } else if constexpr (!FB_PSK_ONLY) {
                        if constexpr (MMSE_BATCH) {
                            d = fold ? pslicer.diff_scaled(z, sc, lane_word(tb.lane, q)) : pslicer.diff(z, lane_word(tb.lane, q));
                        } else {
                            d = pslicer.diff(z, lane_word(tb.lane, q));
                        }
                    }
                    bes += __popc(d);
                    ses += PermSlicer<FB>::nonzero_bytes(d);
#ifdef OFDM_RX_BODY_DENS
                    // DENS: the point k_rx_prof forms for its error vector
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = t + (4 * q + j) * TPS;
                        if (k >= dt.k_lo && k < dt.k_hi)
                            dens_bin<R>(cscale(z[j], fold ? sc[j] * scale : scale), dt, dhist, dout);
                    }
#endif
#ifdef OFDM_RX_BODY_SOFT
                    // SOFT: the point k_rx_prof forms and the lane byte's transmitted index, every bit compared
                    if constexpr (!FB_PSK_ONLY) {
                        const uint32_t stx = lane_word(tb.lane, q) & PermSlicer<FB>::BYTE_MASK;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = t + (4 * q + j) * TPS;
                            if (k >= st.k_lo && k < st.k_hi)
                                soft_bin<FB / 2, R>(cscale(z[j], fold ? sc[j] * scale : scale), FB / 2, (stx >> (8 * j)) & 0xFFu,
                                                    0xFFu, sl_.lev, st.g[k], st, shist, sinv);
                        }
                    }
#endif
                    if constexpr (PROF) {
                        // per element: the counts from its byte of d; the error vector from z times
                        // its MMSE scale (folded into the slicer) and the slicer's 1/sqrt(N), against
                        // the staged LUT point of the lane byte
                        const uint32_t txw = lane_word(tb.lane, q) & PermSlicer<FB>::BYTE_MASK;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t db = (d >> (8 * j)) & 0xFFu;
                            pse[4 * q + j] += db != 0u;
                            pbe[4 * q + j] += __popc(db);
                            prof_power<R>(cscale(z[j], fold ? sc[j] * scale : scale), plut[(txw >> (8 * j)) & 0xFFu],
                                          pl0[4 * q + j], pl1[4 * q + j], pcl[4 * q + j]);
                        }
                    }
                });
            } else {
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const int k = t + i * TPS;
                    const C v = equalized(i);
                    if (sl < a.z_keep) ((C*)a.z_out)[sl * N + k] = v;
                    uint32_t ridx;
                    int b, off;
                    [[maybe_unused]] int loff = 0;  // PROF: the subcarrier's LUT in the pool
                    if (adaptive) {
                        const ScInfo sc = cm.sc[k];
                        if (sc.lut < 0) continue;
                        b = sc.bits;
                        off = sc.bitoff;
                        if constexpr (PROF) loff = axis[sc.lut].lut_off;
                        // PSK orders (constellation/adaptive.py:130-265 with the PSK base mapper):
                        // the nearest point of the subcarrier's own LUT
                        // (a plan with an order above 256: every LUT of it through the wide tables)
                        if constexpr (WIDE)
                            ridx = nn ? nn_decide<R>(v, cm, axis[sc.lut].lut_off, 1 << sc.bits)
                                      : slice_wide<R>(v, axis[sc.lut], lds.wpat + 2 * kWideSide * sc.lut,
                                                      lds.wpat + 2 * kWideSide * sc.lut + kWideSide);
                        else
                            ridx = nn ? nn_decide<R>(v, cm, axis[sc.lut].lut_off, 1 << sc.bits) : slice<R>(v, axis[sc.lut]);
                    } else {
                        b = cm.b;
                        off = k * b;
                        if constexpr (WIDE)
                            ridx = nn ? nn_decide<R>(v, cm, 0, cm.lut_len)
                                      : slice_wide<R>(v, axis[0], lds.wpat, lds.wpat + kWideSide);
                        else
                            ridx = nn ? nn_decide<R>(v, cm, 0, cm.lut_len) : slicer(v);
                    }
#ifdef OFDM_RX_BODY_DENS
                    // DENS: the value the tap stores (an adaptive plan's order-0 subcarrier left above)
                    if (k >= dt.k_lo && k < dt.k_hi) dens_bin<R>(v, dt, dhist, dout);
#endif
                    const uint32_t tidx = tb.generic(i, b, off);
                    uint32_t d = ridx ^ tidx;
                    ses += d != 0u;
                    if constexpr (PROF) pse[i] += d != 0u;
                    if (!all_valid) {
                        const int64_t nvb = a.n_valid_bits - (sbit + off);
                        const int keep = nvb <= 0 ? 0 : (nvb >= b ? b : (int)nvb);
                        d &= ((1u << keep) - 1u) << (b - keep);
                    }
                    bes += __popc(d);
#ifdef OFDM_RX_BODY_SOFT
                    // SOFT: the value the tap stores, the transmitted index and the mask d was compared under
                    // (b / 2 outside 1 .. 4: a memory-safety guard only -- the ABI refuses such a plan, soft_ok)
                    if (k >= st.k_lo && k < st.k_hi && b >= 2 && b <= 8 && !(b & 1)) {
                        uint32_t cmask = 0xFFu;
                        if (!all_valid) {
                            const int64_t nvb = a.n_valid_bits - (sbit + off);
                            const int keep = nvb <= 0 ? 0 : (nvb >= b ? b : (int)nvb);
                            cmask = ((1u << keep) - 1u) << (b - keep);
                        }
                        soft_bin_call<R>(v, b >> 1, tidx, cmask, sl_.lev + (adaptive ? (int)cm.sc[k].lut : 0) * 2 * kSoftSide, st.g[k],
                                         st, shist, sinv);
                    }
#endif
                    if constexpr (PROF) {
                        // error vector against the transmitted point (the plan's LUT pool, plan
                        // precision), its power capped at kProfCap so that fx_accum's share stays
                        // below 2^24; a capped or non-finite sample (ZF on a null bin) is counted
                        pbe[i] += __popc(d);
                        prof_power<R>(v, ((const C*)cm.lut)[loff + (int)tidx], pl0[i], pl1[i], pcl[i]);
                    }
                }
            }
            be += bes;
            se += ses;
#ifdef OFDM_RX_BODY_FRAMES
            // FRAMES: this symbol's counts into its frame.  A lane's share is <= 192 bit and 16 symbol
            // errors and a wave's <= 12288 and 1024, so both fit one word through the sum over the
            // symbol's lanes of this wave (segments of TPS lanes where several symbols share a wave, every
            // lane of a segment active with it; a symbol of 2 / 4 waves adds once per wave).  The first
            // lane of the segment adds the non-zero fields; the frame index: RxFramesTail.
            // (butterflies inside 32 lanes through ds_swizzle's bit mode, xor mask 1 << j, which needs no
            // lane-address register; the two halves of a whole wave through two v_readlane)
            {
                constexpr int SEG = TPS < 64 ? TPS : 64, SEG32 = SEG < 32 ? SEG : 32;
                constexpr int LOGS = SEG32 == 32 ? 5 : SEG32 == 16 ? 4 : SEG32 == 8 ? 3 : SEG32 == 4 ? 2 : SEG32 == 2 ? 1 : 0;
                uint32_t v = bes + (ses << 16);
                static_for<0, LOGS>([&](auto J) {
                    constexpr int pattern = ((1 << J) << 10) | 0x1F;  // and 0x1F, or 0, xor 1 << J
                    v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, pattern);
                });
                if constexpr (SEG == 64)
                    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
                if ((threadIdx.x & (SEG - 1)) == 0 && v) {
#ifdef OFDM_RX_BODY_SWEEP
                    // k_rx_sweep_frames, a symbol of whole waves: v is the wave's sum of the symbol at this
                    // point, which the sweep's own wave sum below would form again -- the workgroup's pair of
                    // the point gets it from here.  (Segments of several symbols per wave: left to that sum.)
                    if constexpr (SEG == 64) {
                        atomicAdd(&lds.scnt[2 * pt], (unsigned long long)(v & 0xFFFFu));
                        atomicAdd(&lds.scnt[2 * pt + 1], (unsigned long long)(v >> 16));
                    }
#endif
                    const uint32_t rel = (uint32_t)sl;
                    const int64_t f = ft.base + (rel < ft.first ? 0 : 1 + (int64_t)((rel - ft.first) / ft.flen));
                    // a memory-safety guard only, never taken: the ABI (frames_ok, the one check of the frame
                    // arguments) refuses a record too short for the call's last symbol before any launch
                    if (f < ft.n_frames) {
                        if (v & 0xFFFFu) atomicAdd(ft.frames + 2 * OFDM_RX_FRAME_ROW(f), (unsigned long long)(v & 0xFFFFu));
                        if (v >> 16) atomicAdd(ft.frames + 2 * OFDM_RX_FRAME_ROW(f) + 1, (unsigned long long)(v >> 16));
                    }
                }
            }
#endif
        }
#ifdef OFDM_RX_BODY_SWEEP
        // this symbol's counts at this point (a lane's: <= 128 bit and 16 symbol errors, so both fit one
        // word through the wave's sum) into the workgroup's pair of the point
        // (k_rx_sweep_frames with a symbol of whole waves: the frame block has added the wave's sum)
        {
            if constexpr (!(FRAMES && TPS >= 64)) {
                unsigned long long v = be | (se << 32);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if ((threadIdx.x & 63) == 0 && v) {
                    atomicAdd(&lds.scnt[2 * pt], v & 0xFFFFFFFFull);
                    atomicAdd(&lds.scnt[2 * pt + 1], v >> 32);
                }
            }
            be = se = 0;
        }
#endif
#ifdef OFDM_RX_BODY_DENS
        // DENS: before a 32-bit bin could wrap (k_rx_dens), the bins go to the record and start again.
        // The iteration count is the workgroup's, so every thread takes the branch together.
        if (--dleft == 0) {
            __syncthreads();
            dens_flush(true);
            __syncthreads();
            dleft = dt.flush;
        }
#endif
#ifdef OFDM_RX_BODY_SOFT
        // SOFT: as DENS -- before a 32-bit bin could wrap, the bins go to the record and start again
        if (--sleft == 0) {
            __syncthreads();
            soft_flush(true);
            __syncthreads();
            sleft = st.flush;
        }
#endif
        sym_sync<TPS>();  // W and the FFT row are rewritten by the next symbol
#ifdef OFDM_RX_BODY_SWEEP
        }  // (the point loop: the next point's FFT rewrites the row too)
#endif
    }
    be = block_sum<unsigned long long, BLK>(be, redc);
    se = block_sum<unsigned long long, BLK>(se, redc);
    if (threadIdx.x == 0) {
        if (be) atomicAdd((unsigned long long*)&a.counters[0], be);
        if (se) atomicAdd((unsigned long long*)&a.counters[1], se);
    }
#ifdef OFDM_RX_BODY_DENS
    // DENS: the workgroup's bins and its outside count into the record
    __syncthreads();
    dens_flush(false);
    dout = block_sum<unsigned long long, BLK>(dout, redc);
    if (threadIdx.x == 0 && dout) atomicAdd(dt.hist + dcells, dout);
#endif
#ifdef OFDM_RX_BODY_SOFT
    // SOFT: the workgroup's bins and its NaN count into the record
    __syncthreads();
    soft_flush(false);
    sinv = block_sum<unsigned long long, BLK>(sinv, redc);
    if (threadIdx.x == 0 && sinv) atomicAdd(st.hist + scells, sinv);
#endif
#ifdef OFDM_RX_BODY_SWEEP
    // (be and se are zero here, and block_sum's barriers stand between the points' LDS sums and this
    // read)  counters[n_snr][2]: one integer atomic pair per point and workgroup
    for (int i = threadIdx.x; i < 2 * n_sweep; i += BLK) {
        const unsigned long long v = lds.scnt[i];
        if (v) atomicAdd((unsigned long long*)&a.counters[i], v);
    }
#endif
    if constexpr (PROF) {
        // row by row: every lane writes its elements into its symbol slot (SPB x N 64-bit words
        // over the FFT rows, which hold at least 8 bytes per element), the slots are summed per
        // subcarrier and the sum added to the record.  The low limb's carry of a subcarrier joins
        // its high limb here, so the record's low row grows by less than 2^32 per workgroup.
        static_assert((SPLIT ? sizeof(R) : sizeof(C)) >= sizeof(unsigned long long), "a 64-bit slot per row element");
        constexpr int KPT = (N + BLK - 1) / BLK;  // subcarriers a thread sums
        unsigned long long* slots = (unsigned long long*)rowmem;
        unsigned long long carry[KPT] = {};
#pragma unroll
        for (int i = 0; i < E; ++i) fx_normalize(pl0[i], pl1[i]);
        static_for<0, kProfRows>([&](auto Rw) {
            constexpr int r = Rw;
            __syncthreads();  // the rows (and the previous round's slots) are free
#pragma unroll
            for (int i = 0; i < E; ++i)
                slots[ls * N + t + i * TPS] = r == 0 ? pbe[i] : r == 1 ? pse[i] : r == 2 ? pl0[i] : r == 3 ? pl1[i] : pcl[i];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const int k = threadIdx.x + j * BLK;
                if (k < N) {
                    unsigned long long sum = 0;
                    for (int q = 0; q < G::SPB; ++q) sum += slots[q * N + k];
                    if constexpr (r == 2) carry[j] = sum >> 32, sum &= 0xFFFFFFFFull;
                    if constexpr (r == 3) sum += carry[j];
                    if (sum) atomicAdd((unsigned long long*)a.profile + (size_t)r * N + k, sum);
                }
            }
        });
    }
#undef OFDM_RX_SNR_LIN
#ifdef OFDM_RX_BODY_FRAMES
#undef OFDM_RX_FRAME_ROW
#endif
