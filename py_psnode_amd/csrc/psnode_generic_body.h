// The body of K0's kernel, as text: generic_kernel (psnode_generic_impl.h) includes this file between its braces.
// Template parameters in scope: DAE, MODE, ML, QM.  Names in scope: a, act (ActPair; NoActPair in the ELU(1) object), rk (read under
// Bd::rk only) and sub (Bd::Sub, read under Bd::sub only); a build whose kernel takes fewer arguments sees an unread default.  The build
// policy Bd decides the rest with `if constexpr`.
    constexpr bool STREAM = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * TB;
    const int xd = a.xd, zd = a.zd;
    const int vd = DAE ? a.vd : 0, id = DAE ? a.id : 0;
    const int n = xd + zd + vd + id;   // width of all_initial
    const int ne = n - xd;             // external rows: z | v | i
    const int nzv = zd + vd;

    // quad-row buffers (float offsets): the two MLP inputs keep their constant columns (a0; the externals of a step) between evaluations,
    // only the columns that change are rewritten -- per stage that is the state x alone
    constexpr int inDE = 0;
    const int SX = de_sx(xd), SA = ae_sa(xd, nzv);      // first column of the second block of the DE / AE input
    const int inAE = de_k16(xd, n) * TB;
    const int ping = inAE + (DAE ? ae_k16(xd, nzv, n) * TB : 0);
    const int pong = ping + up16(a.maxo) * TB;
    float* a0 = lds + pong + up16(a.maxo) * TB;   // [n][TB]
    float* ext = a0 + n * TB;          // [ne][TB] z | v | i fed to the DE stages of this step
    float* xcur = ext + ne * TB;       // [xd][TB] running state
    float* xsrc = xcur + xd * TB;      // [xd][TB] start of this step (xcur, or dataset x under teacher forcing)
    float* kbuf = xsrc + xd * TB;      // [4][xd][TB]
    float* icur = kbuf + 4 * xd * TB;  // [id][TB]
    float* zvn = icur + id * TB;       // [nzv][TB] dataset z | v of the NEXT grid point
    float* dts = zvn + nzv * TB;       // [TB]
    [[maybe_unused]] float* wl = dts + TB;      // Bd::lin only: [nzv][TB] z | v at the interval's left end (the jumped values behind an event)
    [[maybe_unused]] float* wn = dts + TB;      // Bd::lag, in wl's place: [4][nzv][TB] the node rows of the interval's stencil (node 0 jumped where the table says so)

#ifdef PSNODE_K0_PROF      // discriminator builds only: cycles per phase of workgroup 0, printed by its first thread
    long long prof[6] = {0, 0, 0, 0, 0, 0};
    long long pt = clock64();
#define K0_PROF(i) { const long long now_ = clock64(); prof[i] += now_ - pt; pt = now_; }
#else
#define K0_PROF(i)
#endif
    Pref pf;
    pf.tag = nullptr;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned bias_at = (unsigned)(dts + TB - lds) + (Bd::lin ? (unsigned)((Bd::lag ? 4 : 1) * nzv * TB) : 0u), img_at = bias_at + (unsigned)generic_bias_floats(a, DAE);
    const Tab<ML> tde = make_tab<ML>(a.de, wv, a.k0_res & 0xffu, bias_at, img_at, de_k16(xd, n), SX >> 4);
    const Tab<ML> tae = DAE ? make_tab<ML>(a.ae, wv, (a.k0_res >> 8) & 0xffu, bias_at, img_at, ae_k16(xd, nzv, n), SA >> 4) : tde;
    load_resident(a.de, tde, lds);
    if constexpr (DAE) load_resident(a.ae, tae, lds);
    WReg<MODE == 0 ? ML : 2, MODE == 0 ? QM : 1> wde;
    WRegW<MODE == 3 ? ML : 3> wdw;
    if constexpr (MODE == 3) load_regs_wide<ML>(a.de, tde, wdw);
    const f4 fzero = f4{0.f, 0.f, 0.f, 0.f};
    f4 cde = fzero, cde2 = fzero, cae = fzero;       // fold0 of the wave's tile(s) of the DE's / AE's first layer (register forms)
    WReg<(MODE == 0 && DAE) ? ML : 2, (MODE == 0 && DAE) ? QM : 1> wae;
    if constexpr (MODE == 0) {
        load_regs<ML, QM>(a.de, tde, wde);
        if constexpr (DAE) load_regs<ML, QM>(a.ae, tae, wae);
    }

    auto gb = [&](int c) -> long long { const long long b = b0 + c; return b < a.B ? b : a.B - 1; };
    const bool true_x = (a.flags & PSNODE_FLAG_INPUT_TRUE_X) != 0;
    const bool true_i = DAE && (a.flags & PSNODE_FLAG_INPUT_TRUE_I) != 0;
    const int nx = xd * TB;
    // dataset z | v row r of trajectory column c at grid point j
    auto zv_at = [&](long long j, int r, int c) -> float {
        const long long b = gb(c);
        return r < zd ? a.z.p[j * a.z.st + b * a.z.sb + r] : a.v.p[j * a.v.st + b * a.v.sb + (r - zd)];
    };
    // external row r (z | v | i order) of the DE input: columns n + xd + r (s - a0) and 2 n + xd + r (s)
    auto put_ext = [&](int r, int c, float v) {
        ext[r * TB + c] = v;
        lds[inDE + qi(SX + n + r, c)] = v - a0[(xd + r) * TB + c];
        lds[inDE + qi(SX + n + ne + r, c)] = v;
    };
    auto put_x = [&](int r, int c, float v) {
        lds[inDE + qi(r, c)] = v - a0[r * TB + c];
        lds[inDE + qi(xd + r, c)] = v;
    };

    // Segments in parallel (Bd::par): this workgroup runs steps k_lo .. k_hi - 1 alone, the segments of time chunk blockIdx.y.  Chunk 0 starts
    // as every other build does; a later chunk starts on a restart point, so it writes no row 0, runs no pseudo-step, and its first step finds
    // z | v of grid point k_lo where a step finds them "from the previous step's final pass".  (0 and a.T - 1 in every other build.)
    [[maybe_unused]] long long k_lo = 0, k_hi = 0;
    if constexpr (Bd::par) {
        const MspChunk ch = msp_chunk(sub, a.T);
        k_lo = uniform64(ch.k_lo);
        k_hi = uniform64(ch.k_hi);
    }

    // ---- per-trajectory constants, the constant and pad columns of both inputs, the initial state, z | v of grid point 0
    for (int idx = tid; idx < n * TB; idx += NT) {
        const int r = idx / TB, c = idx % TB;
        const float v = a.a0[gb(c) * n + r];
        a0[idx] = v;
        lds[inDE + qi(SX + r, c)] = v;
        if constexpr (DAE) lds[inAE + qi(SA + r, c)] = v;
    }
    for (int idx = tid; idx < de_k16(xd, n) * TB; idx += NT)       // pad columns (the others are overwritten below / at the top of every step)
        if (de_orig_col(idx / TB, xd, n) < 0) lds[inDE + qi(idx / TB, idx % TB)] = 0.0f;
    if constexpr (DAE)
        for (int idx = tid; idx < ae_k16(xd, nzv, n) * TB; idx += NT)
            if (ae_orig_col(idx / TB, xd, nzv, n) < 0) lds[inAE + qi(idx / TB, idx % TB)] = 0.0f;
    for (int idx = tid; idx < nx; idx += NT) {
        const int r = idx / TB, c = idx % TB;
        const long long b = gb(c);
        const float v = DAE ? a.x_init[b * xd + r] : a.x.p[b * a.x.sb + r];
        xcur[idx] = v;
        if constexpr (Bd::par) { if (k_lo > 0) continue; }      // (a later chunk: row 0 is chunk 0's; its first step restarts from a.x[k_lo], its head reads that row)
        if (b0 + c < a.B) a.xo[b * xd + r] = v;
        if constexpr (DAE) lds[inAE + qi(r, c)] = true_x ? a.x.p[b * a.x.sb + r] : v;      // my_solvers.py:95
    }
    for (int idx = tid; idx < nzv * TB; idx += NT) {
        const float v = zv_at(Bd::par ? k_lo : 0, idx / TB, idx % TB);
        zvn[idx] = v;
        if constexpr (DAE) lds[inAE + qi(xd + idx / TB, idx % TB)] = v;
    }
    lds_barrier();

    if constexpr (MODE == 0 && DAE) {       // the AE's a0 block: constant over the trajectory
        if (wv < tab_tiles(tae.dims[0])) cae = fold0<ML>(tae, lds, inAE, wv);
    }
    const int nstage = Bd::rk ? __builtin_amdgcn_readfirstlane(rk.stages) : (a.method == PSNODE_EULER ? 1 : (a.method == PSNODE_MIDPOINT ? 2 : 4));
    // The coefficients go to LDS once: rows a[1][0], a[2][0..1], a[3][0..2], b[0..3] packed into ten floats of kbuf's fourth slot, which no
    // stage pass writes (kbuf keeps k_0 .. k_{S - 2}, at most three slopes; nx >= 16).  Read back per stage pass as broadcasts: kept as kernel
    // arguments they cost the time loop scalar registers it does not have.  (Every step's input barrier lies between this and the first read.)
    static_assert(TB >= 10, "the tableau needs ten floats of the fourth kbuf slot (nx = x_dim * TB)");
    float* rkt = kbuf + 3 * xd * TB;
    if constexpr (Bd::rk) {
        if (tid < 10) rkt[tid] = tid < 6 ? (&rk.a[0][0])[tid == 0 ? 4 : (tid == 1 ? 8 : (tid == 2 ? 9 : 9 + tid))] : rk.b[tid - 6];
    }
    // Sub-steps (Bd::sub): every grid interval runs nsub passes of the evaluation loop on h = (t[k + 1] - t[k]) / nsub with the interval's
    // z | v held; behind a sub-step that is not the interval's last the new state goes where a step's start state lives and nothing else
    // advances.  1 in every other build.
    int nsub = 1;
    // (the sub-step build pins the loop bound in scalar registers: left to the compiler it is reloaded inside the divergent arms below, merges
    //  into a vector register, and the whole time loop then sits under a vector-compare guard)
    long long Tn = 0;
    if constexpr (Bd::sub) {
        nsub = __builtin_amdgcn_readfirstlane(sub.n);
        Tn = uniform64(a.T);
    }
    // look-ahead registers: clocks (threads < TB), the next step's event index, the next grid point's z | v
    float tc = 0.0f, tn = 0.0f;
    if constexpr (Bd::par) {      // (k_lo + 1 <= k_hi <= T - 1 where the record has a step; T == 1: k_lo = k_hi = 0)
        if (tid < TB) {
            tc = a.t.p[k_lo * a.t.st + gb(tid) * a.t.sb];
            tn = a.T > 1 ? a.t.p[(k_lo + 1) * a.t.st + gb(tid) * a.t.sb] : tc;
        }
    } else {
    if (tid < TB) {
        tc = a.t.p[gb(tid) * a.t.sb];
        tn = a.T > 1 ? a.t.p[a.t.st + gb(tid) * a.t.sb] : tc;
    }
    }
    // the next step's event index travels through a VECTOR load (every lane the same address): a scalar load would be waited for by the
    // very next LDS wait (SMEM returns out of order, so any lgkmcnt wait is lgkmcnt(0)) -- an L2 round trip at the top of every step
    const int* evp = a.ev ? a.ev : reinterpret_cast<const int*>(a.t.p);      // (a valid address when there are no events)
    // Per-trajectory events (Bd::pev): the table is [T - 1][B] and every thread carries the index of ITS column -- every loop below walks
    // idx = tid + NT j, so a thread only ever touches column tid % TB -- loaded one step ahead like the shared one.  The host refuses a
    // call of this build without a table.
    static_assert(NT % TB == 0 && TB <= 64 && 64 % TB == 0, "a thread owns one trajectory column, and every wave holds all of them");
    int evn_v = (a.ev && a.T > 1) ? __builtin_nontemporal_load(evp + (Bd::par ? k_lo : 0)) : -1;
    if constexpr (Bd::pev && !Bd::ab) evn_v = a.T > 1 ? evp[gb(tid % TB)] : -1;
    // Adams-Bashforth 2 (Bd::ab; one DE stage per step, one sub-step): x_{k+1} = x_k + c0 f_k + c1 f_{k-1} with per-column c0 / c1 from this
    // step's h, the previous one's (hp, a register of the threads < TB that hold the clocks) and the restart bit (k = 0, an event of the
    // column, hp == 0).  c0 takes h's place in dts; c1 and the previous slope live in kbuf's slots 1 and 0, which a one-stage build never
    // writes.  The event table is read through strides: [T - 1][B], or the shared [T - 1] with a column stride of 0; it may be null.
    [[maybe_unused]] long long ev_sk = 1, ev_sb = 0;
    [[maybe_unused]] float hp = 0.0f;
    if constexpr (Bd::ab) {
        if (ev_table_pt(sub)) { ev_sk = a.B; ev_sb = 1; }
        evn_v = (a.ev && a.T > 1) ? evp[gb(tid % TB) * ev_sb] : -1;
    }
    // Adams-Bashforth 3 (Bd::ab3, on Bd::ab's policy): x_{k+1} = x_k + c0 f_k + c1 f_{k-1} + c2 f_{k-2} with the per-column coefficients of
    // ab3_coef (psnode_generic_build.h) by the depth of the history, and on a restart step (k = 0, an event of the column, h_{k-1} == 0) a Heun
    // corrector on the rows of grid point k + 1: two more evaluation slots, run only where some column of the workgroup restarts, selected
    // per column.  EVERY thread carries the clocks of ITS column (tid % TB: the column of every item a thread touches), the two previous
    // steps, the restart flags and the coefficients in registers -- nothing per column goes through LDS; f_{k-1} / f_{k-2} live in kbuf's
    // slots 0 / 2, written and read by the owning thread alone.
    [[maybe_unused]] float ab_h0 = 0.0f, ab_h1 = 0.0f, ab_h2 = 0.0f, ab_c0 = 0.0f, ab_c1 = 0.0f, ab_c2 = 0.0f;
    [[maybe_unused]] bool ab_rs = true, ab_rp = true, any_rs = false;
    if constexpr (Bd::ab3) {
        tc = a.t.p[gb(tid % TB) * a.t.sb];
        tn = a.T > 1 ? a.t.p[a.t.st + gb(tid % TB) * a.t.sb] : tc;
    }

    // Multiple shooting (Bd::ms): grid point k > 0 with k % every == 0 is a restart point -- the step that leaves it starts from the dataset
    // row a.x[k] and, in a DAE, feeds the DE the head at that row (the event slot, which then runs without an event too).  Launch-uniform:
    // ms_cnt counts the steps since the last restart in a scalar register, so no step pays a 64-bit remainder.
    [[maybe_unused]] int ms_cnt = 0, ms_w = 0;
    if constexpr (Bd::ms) ms_w = __builtin_amdgcn_readfirstlane(ms_every(sub));
    if constexpr (Bd::par) { if (k_lo > 0) ms_cnt = ms_w; }      // (a later chunk's first step leaves a restart point)

    // Stage-wise algebraic heads (Bd::sth, on Bd::lin's policy; DAE): behind a stage pass that is not the (sub-)step's last the head runs at the
    // next stage's argument and externals -- the pass writes both into the AE input as well -- and its result becomes the i columns of the DE
    // input, the way the in-interval head in front of a sub-step does.  sth_hd: the evaluation about to run is such a head (workgroup-uniform).
    [[maybe_unused]] bool sth_hd = false;
    float pz[PF];
    // Linear externals (Bd::lin): stage s of sub-step j reads z | v at theta = (j + c_s) / nsub between the interval's left rows (wl) and the
    // dataset's rows of grid point k + 1 (zvn, which the first stage pass of the interval fills from the look-ahead registers).  th_in: the
    // theta of the rows the DE input holds; th_fd: the one the register forms' fold0 was taken at.  Both are wave-uniform.
    [[maybe_unused]] float th_in = 0.0f, th_fd = 0.0f;
    // Lagrange externals (Bd::lag, on Bd::lin's policy): the same passes, with the polynomial through the q <= 4 node rows of the column's
    // stencil (lag_stencil, psnode_generic_build.h) in the straight line's place.  Every thread carries the stencil of ITS column (tid % TB:
    // the column of every item a thread touches); the node rows go to wn behind the interval's first evaluation, whose theta is 0 -- the
    // left rows themselves.  The weights are per thread, theta is wave-uniform.  Like the other look-ahead values the code byte is loaded
    // one interval ahead (lag_cn) and the node rows of a thread's first item are requested at the top of the step (pn): their latency -- the
    // event index at the first node, then the rows -- hides behind the first evaluation.
    [[maybe_unused]] LagStencil lag_st{0, 2, 0};
    [[maybe_unused]] int lag_cn = 0, lag_evs = -1;
    [[maybe_unused]] float pn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (Bd::lag) { if (a.T > 1) lag_cn = lag_code(lag_table(sub), 0, a.B, gb(tid % TB)); }

    // One MLP call site for every evaluation (the unrolled layer code exists once: it has to stay inside the instruction cache).  Slots of
    // step k: 0 = the AE head at an event (my_solvers.py:110), 1 .. S = the DE stages, S + 1 = the AE head at grid point k + 1
    // (my_solvers.py:95, 121); the pseudo-step k = -1 of the DAE is that last slot alone, for grid point 0.
    for (long long k = Bd::par ? ((DAE && k_lo == 0) ? -1 : k_lo) : (DAE ? -1 : 0); Bd::par ? k < k_hi : k + 1 < (Bd::sub ? Tn : a.T); ++k) {
        K0_PROF(5)
        // ev: the event index of this step -- launch-uniform, or (Bd::pev) this thread's column's; any_ev: some trajectory of the workgroup
        // has one (workgroup-uniform: each wave holds every column), which is what decides whether the event slot runs
        // (the constant conditions on Bd::pev keep the statements of the other builds where they were: their code does not change)
        const int ev = k >= 0 ? (Bd::pev ? evn_v : __builtin_amdgcn_readfirstlane(evn_v)) : -1;
        [[maybe_unused]] bool any_ev = false;
        if constexpr (Bd::pev) any_ev = __builtin_amdgcn_ballot_w64(ev >= 0) != 0;
        [[maybe_unused]] bool ms_rs = false;      // (Bd::ms) this step leaves a restart point
        if constexpr (Bd::ms) {
            if (k >= 0) {
                ms_rs = ms_cnt == ms_w;      // (k == 0: ms_cnt is 0 and every >= 1)
                ms_cnt = __builtin_amdgcn_readfirstlane(ms_rs ? 1 : ms_cnt + 1);
            }
        }
        if (k >= 0) {
            // ---- this step's inputs (zero-order hold: the left grid point feeds every stage)
            if constexpr (Bd::ab3) {      // (every thread, for its column tid % TB: `ev` is that column's)
                ab_h2 = ab_h1;
                ab_h1 = ab_h0;
                ab_rp = ab_rs;
                ab_h0 = tn - tc;
                ab_rs = k == 0 || ev >= 0 || ab_h1 == 0.0f;
                const Ab3Coef cf = ab3_coef(ab_h0, ab_h1, ab_h2, ab_rs, ab_rp || ab_h1 + ab_h2 == 0.0f);
                ab_c0 = cf.c0;
                ab_c1 = cf.c1;
                ab_c2 = cf.c2;
                any_rs = __builtin_amdgcn_ballot_w64(ab_rs) != 0;      // (workgroup-uniform: each wave holds every column)
            } else if constexpr (Bd::ab) {
                if (tid < TB) {      // (a thread < TB owns column tid: `ev` is that column's)
                    const float h = tn - tc;
                    const bool restart = k == 0 || ev >= 0 || hp == 0.0f;
                    const float half_rho = (h / hp) / 2.0f;
                    dts[tid] = restart ? h : h * (1.0f + half_rho);
                    kbuf[nx + tid] = restart ? 0.0f : -(h * half_rho);
                    hp = h;
                }
            } else if constexpr (Bd::sub) { if (tid < TB) dts[tid] = Bd::rkc ? tn - tc : (tn - tc) / (float)nsub; }
            else { if (tid < TB) dts[tid] = tn - tc; }
            for (int idx = tid; idx < nzv * TB; idx += NT) {
                const int r = idx / TB, c = idx % TB;
                float v;
                if (ev >= 0) { const long long b = gb(c); v = r < zd ? a.zj[b * a.zjb + ev * a.zje + r] : a.vj[b * a.vjb + ev * a.vje + (r - zd)]; }
                else v = zvn[idx];
                put_ext(r, c, v);
                if constexpr (Bd::lin && !Bd::lag) wl[idx] = v;
                if constexpr (DAE) if (ev >= 0) lds[inAE + qi(xd + r, c)] = v;      // the event's AE evaluation sees the jumped rows
            }
            if constexpr (Bd::lin) th_in = 0.0f;
            if constexpr (Bd::lag) {
                lag_st = lag_decode(lag_cn, k, a.T);
                lag_cn = k + 2 < a.T ? lag_code(lag_table(sub), k + 1, a.B, gb(tid % TB)) : 0;
                if (nstage > 1 || nsub > 1) {      // (a one-stage, one-sub-step interval reads theta = 0 alone)
                    // the stencil's node rows of this thread's first item: dataset rows lag_st.s .. + q - 1 of its column, node 0 from the
                    // jump rows where the event table has an event at step s (0 beyond q); every lane loads, from a valid address
                    lag_evs = a.ev ? evp[lag_st.s] : -1;
                    const int ii = tid < nzv * TB ? tid : 0, r = ii / TB, c = ii % TB;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        float v = 0.0f;
                        if (nzv > 0 && m < lag_st.q) {
                            if (m == 0 && lag_evs >= 0) { const long long b = gb(c); v = r < zd ? a.zj[b * a.zjb + lag_evs * a.zje + r] : a.vj[b * a.vjb + lag_evs * a.vje + (r - zd)]; }
                            else v = zv_at(lag_st.s + m, r, c);
                        }
                        pn[m] = v;
                    }
                }
            }
            for (int idx = tid; idx < nx; idx += NT) {
                const int r = idx / TB, c = idx % TB;
                const float v = (Bd::ms ? ms_rs : true_x) ? a.x.p[k * a.x.st + gb(c) * a.x.sb + r] : xcur[idx];
                xsrc[idx] = v;
                put_x(r, c, v);
                if constexpr (Bd::ms) {      // (the restart head reads the dataset row, an event's inside a segment the computed state)
                    if constexpr (DAE) if (ev >= 0 || ms_rs) lds[inAE + qi(r, c)] = v;
                } else {
                if constexpr (DAE) if (ev >= 0) lds[inAE + qi(r, c)] = xcur[idx];   // ... and the computed state
                }
            }
            if constexpr (DAE) {
                if (ev < 0 && !(Bd::ms && ms_rs))
                    for (int idx = tid; idx < id * TB; idx += NT) {
                        const int r = idx / TB, c = idx % TB;
                        put_ext(nzv + r, c, true_i ? a.i.p[k * a.i.st + gb(c) * a.i.sb + r] : icur[idx]);
                    }
            }
            // ---- look-ahead for grid point k + 1
            const long long k1 = k + 1, k2 = k + 2 < a.T ? k + 2 : a.T - 1;
            if constexpr (Bd::ab3) { tc = tn; tn = a.t.p[k2 * a.t.st + gb(tid % TB) * a.t.sb]; }
            else
            if (tid < TB) { tc = tn; tn = a.t.p[k2 * a.t.st + gb(tid) * a.t.sb]; }
            evn_v = (a.ev && k1 + 1 < a.T) ? evp[k1] : -1;
            if constexpr (Bd::pev && !Bd::ab) evn_v = k1 + 1 < a.T ? evp[k1 * a.B + gb(tid % TB)] : -1;
            if constexpr (Bd::ab) evn_v = (a.ev && k1 + 1 < a.T) ? evp[k1 * ev_sk + gb(tid % TB) * ev_sb] : -1;
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int idx = tid + NT * j;
                const int ii = idx < nzv * TB ? idx : 0;
                pz[j] = nzv > 0 ? zv_at(k1, ii / TB, ii % TB) : 0.0f;
            }
            lds_barrier();
        }
        K0_PROF(0)
        // sub-step si.i of the interval (one pass in the builds without sub-steps, and for the DAE's pseudo-step): only the first has the
        // event slot, only the last the head at grid point k + 1; the others of a DAE that integrates its own i start with an AE evaluation
        // in the event slot's form -- the algebraic variable follows the state inside the interval
        SubIter<Bd::sub> si(k >= 0 ? nsub : 1);
        do {
        // (Bd::ab3: slot 2 = the AE head at the predictor x~ and rows k + 1, slot 3 = the corrector's DE stage -- both only where some column
        //  restarts --, slot 4 = the AE head at grid point k + 1)
        const int e_end = Bd::ab3 ? (DAE ? 4 : (any_rs ? 3 : 1)) : ((DAE && si.last()) ? nstage + 1 : nstage);
        for (int e = k < 0 ? (Bd::ab3 ? 4 : nstage + 1) : ((DAE && (si.first() ? (Bd::pev ? any_ev : (ev >= 0 || (Bd::ms && ms_rs))) : !true_i)) ? 0 : 1); e <= e_end; ++e) {
            if constexpr (Bd::ab3) { if ((e == 2 && !(DAE && any_rs)) || (e == 3 && !any_rs)) continue; }
            // (a constant selects the arm: the builds without stage heads keep the expression they had)
            const bool is_ae = Bd::sth ? (DAE && (e == 0 || e == nstage + 1 || sth_hd))
                                       : (DAE && (e == 0 || e == (Bd::ab3 ? 4 : nstage + 1) || (Bd::ab3 && e == 2)));
            // (Bd::sth: a stage head stands between the stages s and s + 1, so the AE follows every DE stage and the DE every stage head)
            const bool ae_next = Bd::ab3 ? (DAE && (e == 1 || e == 3))
                                         : (Bd::sth ? (DAE && !sth_hd && e >= 1 && (e == nstage ? (si.last() || !true_i) : !true_i))
                                                    : (DAE && e == nstage && (si.last() || !true_i)));
            int f;
            if constexpr (MODE == 0 || MODE == 3) {
                // (sub-steps: the externals change inside an interval only where the DAE's own i does)
                // (linear externals: and in front of every stage whose theta is not the one folded)
                if ((e == 1 && (si.first() || (DAE && !true_i))) || (Bd::lin && !is_ae && th_in != th_fd) || (Bd::ab3 && e == 3) ||
                    (Bd::sth && DAE && !is_ae && e > 1 && !true_i)) {      // (Bd::sth: the i columns changed in front of this stage)       // the step's externals are in place (behind an event's AE evaluation too): the DE's per-step constant
                    const int nt0 = tab_tiles(tde.dims[0]);
                    if (wv < nt0) cde = fold0<ML>(tde, lds, inDE, wv);
                    if (MODE == 3 && wv + 4 < nt0) cde2 = fold0<ML>(tde, lds, inDE, wv + 4);
                    if constexpr (Bd::lin) th_fd = th_in;
                }
            }
            if constexpr (MODE == 3) {
                f = mlp_regw<ML>(tde, lds, inDE, ping, pong, wdw, cde, cde2, ActCtx{act.de});
            } else if constexpr (MODE == 0) {      // two call sites: the operands are two different register sets
                if (is_ae) { if constexpr (DAE) f = mlp_reg<ML, QM>(tae, lds, inAE, ping, pong, wae, cae, ActCtx{act.ae}); else f = ping; }
                else f = mlp_reg<ML, QM>(tde, lds, inDE, ping, pong, wde, cde, ActCtx{act.de});
            } else {
                f = DAE ? mlp_eval<STREAM, ML>(pick_tab(is_ae, tae, tde), lds, is_ae ? inAE : inDE, ping, pong, pf, pick_tab(ae_next, tae, tde),
                                               ActCtx{act_pick(is_ae, act.ae, act.de)})
                        : mlp_eval<STREAM, ML>(tde, lds, inDE, ping, pong, pf, tde, ActCtx{act.de});
            }
            K0_PROF(2)
            if (is_ae) {
                if constexpr (DAE && Bd::sth) {
                    if (sth_hd) {      // i_s = g(X_s; z | v at theta_s): the algebraic input of stage e, no output row; the loop comes back to e
                        for (int idx = tid; idx < id * TB; idx += NT) put_ext(nzv + idx / TB, idx % TB, lds[f + qi(idx / TB, idx % TB)]);
                        lds_barrier();
                        sth_hd = false;
                        --e;
                        K0_PROF(4)
                        continue;
                    }
                }
                if constexpr (DAE) {
                    for (int idx = tid; idx < id * TB; idx += NT) {
                        const int r = idx / TB, c = idx % TB;
                        const float v = lds[f + qi(r, c)];
                        if constexpr (Bd::ab3) { if (e == 2) { put_ext(nzv + r, c, v); continue; } }      // i~: the corrector's algebraic input, no output
                        // (per-trajectory events: the event-time head ran because SOME column has a hit; the others keep the i they carry)
                        if constexpr (Bd::pev) { if (e == 0 && si.first() && ev < 0) continue; }
                        icur[idx] = v;       // read back by the same thread (below, or at the top of the next step)
                        if (e == 0) put_ext(nzv + r, c, true_i ? a.i.p[k * a.i.st + gb(c) * a.i.sb + r] : v);
                        else if (b0 + c < a.B) a.io[((k + 1) * a.B + b0 + c) * id + r] = v;
                    }
                    if (e == 0 || (Bd::ab3 && e == 2)) lds_barrier();
                }
                K0_PROF(4)
                continue;
            }
            // ---- stage s: ONE pass that forms the next stage's argument straight into the DE input (my_fixed_grid.py:15-18, 23-32, 38-51)
            //      or, behind the last stage, the new state, its output row, the AE input and the look-ahead rows
            if constexpr (Bd::ab3) {
                // e == 1: the step's one stage -- the multistep update with this thread's coefficients (a restart column: c0 = h, the Euler
                // predictor x~) -- which shifts the slope history; where some column restarts, x~ and the rows of grid point k + 1 become the
                // next evaluations' inputs instead of the step's result.  e == 3: the corrector, taken by the restart columns alone.
                const bool corr = e == 3;
                const bool pred = !corr && any_rs;
                for (int idx = tid; idx < nx; idx += NT) {
                    const int r = idx / TB, c = idx % TB;
                    const float x0 = xsrc[idx];
                    const float ks = lds[f + qi(r, c)];
                    float v;
                    if (!corr) {      // (c1 / c2 are 0 where the history is not read: its slots may be unwritten)
                        v = x0 + ab_c0 * ks;
                        if (ab_c1 != 0.0f) v = v + ab_c1 * kbuf[idx];
                        if (ab_c2 != 0.0f) v = v + ab_c2 * kbuf[2 * nx + idx];
                        kbuf[2 * nx + idx] = kbuf[idx];
                        kbuf[idx] = ks;          // f_k, the slope kept for the history (never the corrector's)
                    } else {
                        v = ab_rs ? x0 + (ab_h0 * 0.5f) * (kbuf[idx] + ks) : xcur[idx];
                    }
                    xcur[idx] = v;
                    if (pred) put_x(r, c, v);
                    else if (b0 + c < a.B) a.xo[((k + 1) * a.B + b0 + c) * xd + r] = v;
                    if constexpr (DAE) lds[inAE + qi(r, c)] = v;
                }
                if (!corr) {      // z | v of grid point k + 1: the next step's rows, the heads' -- and the corrector's, never jumped
#pragma unroll
                    for (int j = 0; j < PF; ++j) {
                        const int idx = tid + NT * j;
                        if (idx < nzv * TB) {
                            zvn[idx] = pz[j];
                            if constexpr (DAE) lds[inAE + qi(xd + idx / TB, idx % TB)] = pz[j];
                            if (pred) put_ext(idx / TB, idx % TB, pz[j]);
                        }
                    }
                    for (int idx = tid + NT * PF; idx < nzv * TB; idx += NT) {
                        const float v = zv_at(k + 1, idx / TB, idx % TB);
                        zvn[idx] = v;
                        if constexpr (DAE) lds[inAE + qi(xd + idx / TB, idx % TB)] = v;
                        if (pred) put_ext(idx / TB, idx % TB, v);
                    }
                }
                lds_barrier();
                K0_PROF(3)
                continue;
            }
            const int s_ = e - 1;
            const bool final_stage = s_ + 1 == nstage;
            // Runge-Kutta-Chebyshev (Bd::rkc; one evaluation per pass, nsub = the stage count): pass si.i forms Y_j, j = si.i + 1, from Y_0, Y_{j-1},
            // Y_{j-2}, F_0 and the fresh slope.  Y_{j-1} is where a sub-step's start state lives (xsrc); Y_0, Y_{j-2} and F_0 take kbuf's slots
            // 0, 1 and 2, which a one-stage pass never writes -- each element written and read by the thread that owns it.
            [[maybe_unused]] RkcCoef rc{};
            if constexpr (Bd::rkc) rc = rkc_coef(sub, si.i);
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
            if constexpr (Bd::rk) {
            // the tableau row this pass applies to k_0 .. k_s (uniform): a[s + 1][.] -- the next stage's argument -- or, behind the last
            // stage, b.  kbuf keeps k_0 .. k_{S - 2}: at most three slopes.
            auto rku = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
            const float* rrow = rkt + (final_stage ? 6 : (s_ == 0 ? 0 : (s_ == 1 ? 1 : 3)));
            c0 = rku(rrow[0]);
            c1 = s_ >= 1 ? rku(rrow[1]) : 0.0f;
            c2 = s_ >= 2 ? rku(rrow[2]) : 0.0f;
            c3 = s_ >= 3 ? rku(rrow[3]) : 0.0f;
            }
            if constexpr (Bd::lin) {
                if (s_ == 0 && si.first()) {      // the right rows, behind the interval's first evaluation (the final pass rewrites the same values)
#pragma unroll
                    for (int j = 0; j < PF; ++j) {
                        const int idx = tid + NT * j;
                        if (idx < nzv * TB) zvn[idx] = pz[j];
                    }
                    for (int idx = tid + NT * PF; idx < nzv * TB; idx += NT) zvn[idx] = zv_at(k + 1, idx / TB, idx % TB);
                    if constexpr (Bd::lag) {
                        if (!(final_stage && si.last())) {      // (a one-stage, one-sub-step interval reads theta = 0 alone)
                            // the node rows: a thread's first item from the look-ahead registers, items beyond them loaded here
                            if (tid < nzv * TB) {
#pragma unroll
                                for (int m = 0; m < 4; ++m) wn[m * nzv * TB + tid] = pn[m];
                            }
                            for (int idx = tid + NT; idx < nzv * TB; idx += NT) {
                                const int r = idx / TB, c = idx % TB;
#pragma unroll
                                for (int m = 0; m < 4; ++m) {
                                    float v = 0.0f;
                                    if (m < lag_st.q) {
                                        if (m == 0 && lag_evs >= 0) { const long long b = gb(c); v = r < zd ? a.zj[b * a.zjb + lag_evs * a.zje + r] : a.vj[b * a.vjb + lag_evs * a.vje + (r - zd)]; }
                                        else v = zv_at(lag_st.s + m, r, c);
                                    }
                                    wn[m * nzv * TB + idx] = v;
                                }
                            }
                        }
                    }
                }
                if (!(final_stage && si.last())) {
                    // the externals of the next stage, or of the next sub-step's first one (and of the head in front of it): c_{s + 1} is the
                    // row sum just read, in increasing index
                    const float th = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(((float)si.i + (final_stage ? 1.0f : (c0 + c1) + c2)) / (float)nsub)));
                    [[maybe_unused]] LagW lw{};
                    if constexpr (Bd::lag) lw = lag_weights(lag_st.off, lag_st.q, th);
                    for (int idx = tid; idx < nzv * TB; idx += NT) {      // (each thread reads back what it wrote itself)
                        const int r = idx / TB, c = idx % TB;
                        float v;
                        if constexpr (Bd::lag) {
                            v = lag_eval(lw, lag_st.q, wn[idx], wn[nzv * TB + idx], wn[2 * nzv * TB + idx], wn[3 * nzv * TB + idx]);
                        } else {
                        const float l_ = wl[idx];
                        v = l_ + th * (zvn[idx] - l_);
                        }
                        put_ext(r, c, v);
                        if constexpr (DAE) if (final_stage || Bd::sth) lds[inAE + qi(xd + r, c)] = v;      // (Bd::sth: the stage head's rows)
                    }
                    th_in = th;
                }
            }
            for (int idx = tid; idx < nx; idx += NT) {
                const int r = idx / TB, c = idx % TB;
                const float h = dts[c];
                const float x0 = xsrc[idx];
                const float ks = lds[f + qi(r, c)];
                float v;
                if constexpr (Bd::rkc) {
                    // the terms in the order written, a coefficient that is exactly 0 skipped (psnode_rkc_f32); x0 is Y_{j-1}
                    if (si.first()) {
                        kbuf[idx] = x0;
                        kbuf[2 * nx + idx] = ks;
                        v = x0 + (rc.mut * h) * ks;
                    } else {
                        v = rc.mu * x0;
                        if (rc.kap != 0.0f) v = rc.kap * kbuf[idx] + v;
                        if (rc.nu != 0.0f) v = v + rc.nu * kbuf[nx + idx];
                        v = v + (rc.mut * h) * ks;
                        if (rc.gam != 0.0f) v = v + (rc.gam * h) * kbuf[2 * nx + idx];
                    }
                    kbuf[nx + idx] = x0;
                } else
                if constexpr (Bd::rk) {
                // v = x0 + h * sum_j c_j k_j in increasing j, zero coefficients skipped (psnode_rk_tableau_f32); k_s is this stage's slope
                if (s_ < 3 && !final_stage) kbuf[s_ * nx + idx] = ks;
                float acc = 0.0f;
                if (c0 != 0.0f) acc += c0 * (s_ == 0 ? ks : kbuf[idx]);
                if (c1 != 0.0f) acc += c1 * (s_ == 1 ? ks : kbuf[nx + idx]);
                if (c2 != 0.0f) acc += c2 * (s_ == 2 ? ks : kbuf[2 * nx + idx]);
                if (c3 != 0.0f) acc += c3 * ks;
                v = x0 + h * acc;
                if constexpr (Bd::ab) {      // h is this column's c0 and acc the slope (b = {1}); c1 is 0 on a restart step, where slot 0 may be unwritten
                    const float c1_ = kbuf[nx + c];
                    if (c1_ != 0.0f) v = v + c1_ * kbuf[idx];
                    kbuf[idx] = ks;          // f_k for step k + 1: written and read by this thread alone
                }
                } else {
                if (a.method == PSNODE_EULER) {
                    v = x0 + h * ks;
                } else if (a.method == PSNODE_MIDPOINT) {
                    v = s_ == 0 ? x0 + ks * (0.5f * h) : x0 + h * ks;
                } else {
                    if (s_ < 3) kbuf[s_ * nx + idx] = ks;
                    const float k1 = kbuf[idx];
                    if (s_ == 0) v = x0 + h * k1 * kOneThird;
                    else if (s_ == 1) v = x0 + h * (ks - k1 * kOneThird);
                    else if (s_ == 2) v = x0 + h * (k1 - kbuf[nx + idx] + ks);
                    else v = x0 + (k1 + 3.0f * (kbuf[nx + idx] + kbuf[2 * nx + idx]) + ks) * h * 0.125f;
                }
                }
                if (!final_stage) {
                    put_x(r, c, v);
                    if constexpr (DAE && Bd::sth) lds[inAE + qi(r, c)] = v;      // X_{s + 1}, the stage head's state
                } else {
                    if constexpr (Bd::sub) {
                        if (!si.last()) {      // the start state of sub-step si.i + 1: nothing of grid point k + 1 is touched
                            xsrc[idx] = v;
                            xcur[idx] = v;
                            put_x(r, c, v);
                            if constexpr (DAE) lds[inAE + qi(r, c)] = v;
                            if (sub.x_sub && b0 + c < a.B) sub.x_sub[((k * (nsub - 1) + si.i) * a.B + b0 + c) * xd + r] = v;
                            continue;
                        }
                    }
                    xcur[idx] = v;
                    if (b0 + c < a.B) a.xo[((k + 1) * a.B + b0 + c) * xd + r] = v;
                    if constexpr (DAE) lds[inAE + qi(r, c)] = true_x ? a.x.p[(k + 1) * a.x.st + gb(c) * a.x.sb + r] : v;   // my_solvers.py:121
                }
            }
            if (final_stage && si.last()) {
#pragma unroll
                for (int j = 0; j < PF; ++j) {
                    const int idx = tid + NT * j;
                    if (idx < nzv * TB) {
                        zvn[idx] = pz[j];
                        if constexpr (DAE) lds[inAE + qi(xd + idx / TB, idx % TB)] = pz[j];
                    }
                }
                for (int idx = tid + NT * PF; idx < nzv * TB; idx += NT) {
                    const float v = zv_at(k + 1, idx / TB, idx % TB);
                    zvn[idx] = v;
                    if constexpr (DAE) lds[inAE + qi(xd + idx / TB, idx % TB)] = v;
                }
            }
            if constexpr (DAE && Bd::sth) { if (!final_stage && !true_i) sth_hd = true; }
            lds_barrier();
            K0_PROF(3)
        }
        } while (si.more());
    }
#ifdef PSNODE_K0_PROF
    if (blockIdx.x == 0 && tid == 0)
        printf("K0 phases (cycles of clock64, workgroup 0): step inputs %lld | mlp %lld | update %lld | AE head + output %lld | loop %lld\n", prof[0], prof[2],
               prof[3], prof[4], prof[5]);
#endif
#undef K0_PROF
