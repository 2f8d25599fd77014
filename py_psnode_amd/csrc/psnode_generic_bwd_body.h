// The body of K5's kernel, as text: generic_backward_kernel (psnode_generic_bwd_impl.h) includes this file between its braces.
// Template parameters in scope: gg, REG, ggA, STR.  Names in scope: a, act (ActPair; NoActPair in the ELU(1) object), rk (read under
// Bd::rk only) and sub (Bd::Sub, read under Bd::sub only); a build whose kernel takes fewer arguments sees an unread default.
    constexpr bool DE_TM = REG || STR == 2;      // the DE's LDS accumulators are tile-major
    constexpr bool AE_TM = STR >= 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * TB;
    // Segments in parallel (Bd::par): this workgroup sweeps steps k_hi - 1 .. k_lo alone, the segments of time chunk blockIdx.y; wg is its slice
    // of the per-workgroup partials (tiles x chunks of them).  The sweep of a chunk c > 0 ends on the restart step at k_lo, behind which the
    // sequential sweep carries nothing but grad_xs[k_lo] / grad_is[k_lo] -- what chunk c - 1 reads for itself.
    [[maybe_unused]] long long k_lo = 0, k_hi = 0;
    [[maybe_unused]] bool last_chunk = true;
    if constexpr (Bd::par) {
        const MspChunk ch = msp_chunk(sub, a.T);
        k_lo = ch.k_lo;
        k_hi = ch.k_hi;
        last_chunk = blockIdx.y + 1 == gridDim.y;
    }
    // (Bd::ab3 pins the grid length in scalar registers up here, in front of the first divergent loop: read where Bd::ab pins it, below,
    //  the value reaches that place through both arms of the loop guard in a vector register, and the spills of the longer set-up in
    //  front of the sweep then count as stored under partial EXEC)
    [[maybe_unused]] long long T3 = 0;
    if constexpr (Bd::ab3) {
        const unsigned long long u = (unsigned long long)a.T;
        T3 = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u));
    }
    [[maybe_unused]] const size_t wg = Bd::par ? (size_t)blockIdx.y * gridDim.x + blockIdx.x : (size_t)blockIdx.x;
    const bool dae = a.dae != 0;
    const int xd = a.xd, zd = a.zd, vd = dae ? a.vd : 0, id = dae ? a.id : 0;
    const int nzv = zd + vd, ne = nzv + id, n = xd + ne;
    const int S = Bd::rk ? __builtin_amdgcn_readfirstlane(rk.stages) : rk_stages(a.method);
    const int nx = xd * TP;
    // sub-steps per grid interval (Bd::sub; 1 in every other build): the sweep walks them backwards inside each interval, from the start
    // states K0 left in sub.x_sub
    int nsub = 1;
    if constexpr (Bd::sub) nsub = __builtin_amdgcn_readfirstlane(sub.n);
    // teacher forcing: tx -- every DE step and every grid-point head reads the dataset row (xsrc), the adjoint of a step's start state is
    // dropped; ti -- the DE reads i_true[k], its algebraic adjoint is dropped and the event-time head feeds nothing
    const bool tx = (a.flags & PSNODE_FLAG_INPUT_TRUE_X) != 0, ti = dae && (a.flags & PSNODE_FLAG_INPUT_TRUE_I) != 0;
    const float* __restrict__ xsrc = tx ? a.xt : a.xs;
    // Stage-wise algebraic heads (Bd::sth, on Bd::lin's policy): K0 evaluated i_s = g(X_s; z | v at theta_s) in front of every stage s >= 1 of a
    // (sub-)step.  (3a) recomputes them in K0's order and expressions; (3b) recomputes i_s in front of stage s's VJP (no LDS keeps them) and
    // sends the i part of that VJP through the head's VJP at (X_s, ext(theta_s)) -- its x part is the adjoint of X_s, its z | v part goes where
    // the stage's own external adjoint goes, a0 and the AE's parameters where the in-interval head's go.  gic (free between (1) and (4)) keeps
    // stage 0's i meanwhile, gxc (spent once (3b) has read it) takes the head VJP's x part.  Fixed ownership: every element is added by the
    // thread that owns it in the loops around.
    [[maybe_unused]] const bool sth_on = Bd::sth && dae && !ti && S > 1;

    float* acts = lds;                            // [act_rows][TP]
    float* dA = acts + a.act_rows * TP;           // [maxw][TP]
    float* dB = dA + a.maxw * TP;
    float* a0s = dB + a.maxw * TP;                // [n][TP]
    float* ga0s = a0s + n * TP;                   // [n][TP]
    float* ext = ga0s + n * TP;                   // [ne][TP]  z | v | i fed to the DE of this step
    float* gext = ext + ne * TP;                  // [ne][TP]
    float* x0 = gext + ne * TP;                   // [xd][TP]
    float* xst = x0 + nx;                         // [4][xd][TP]
    float* ks = xst + 4 * nx;                     // [4][xd][TP]
    float* gks = ks + 4 * nx;                     // [4][xd][TP]
    float* gx0 = gks + 4 * nx;                    // [xd][TP]
    float* gxc = gx0 + nx;                        // [xd][TP]  carried dL/dx_{k+1}
    float* gic = gxc + nx;                        // [id][TP]  carried dL/di_{k+1}
    float* dts = gic + id * TP;                   // [TP]
    // Linear externals (Bd::lin): the interval's left z | v rows (the jumped values behind an event), the dataset's rows of grid point k + 1,
    // and the adjoint of those right rows -- gext's z | v rows are the left one.  ext's z | v rows are rewritten per stage from the first two.
    [[maybe_unused]] float* wl = dts + TP;                        // [nzv][TP]
    [[maybe_unused]] float* wr = wl + nzv * TP;                   // [nzv][TP]
    [[maybe_unused]] float* gexr = wr + nzv * TP;                 // [nzv][TP]
    // Lagrange externals (Bd::lag, in those three regions' place and five more): the node rows of the interval's stencil (node 0 jumped where
    // the event table has an event at step s) and their adjoints, which (4) adds to the rows s .. s + q - 1 of grad_z / grad_v.  Every thread
    // carries the stencil of ITS column (tid % TB: the column of every TILE_LOOP item of a thread) and the event index at its first node.
    [[maybe_unused]] float* wn = dts + TP;                        // [4][nzv][TP]
    [[maybe_unused]] float* gn = wn + 4 * nzv * TP;               // [4][nzv][TP]
    [[maybe_unused]] LagStencil lag_st{0, 2, 0};
    [[maybe_unused]] int lag_evs = -1;
    float* wbuf = dts + TP + (Bd::lin ? 3 * nzv * TP : 0) + (Bd::lag ? 5 * nzv * TP : 0);        // [kWBuf] staged weights
    // [np_de + np_ae]: in LDS when it fits, else this workgroup's partial slice in global memory (each element is owned by
    // one thread either way, so the read-modify-write needs no atomics)
    float* gacc_g = a.wpart + (Bd::par ? wg : (size_t)blockIdx.x) * (a.de.np + (a.dae ? a.ae.np : 0));      // (used when gg)
    const bool stages = (!REG && STR != 2) || (a.dae && STR == 0);      // some MLP still stages its weights through LDS
    float* gacc_l = wbuf + (stages ? kWBuf : 0);
    // register path of the DE: quad-row buffers behind the accumulators, the wave's MFMA operands of both passes in VGPRs
    const int de_acc = (DE_TM && !gg) ? tm_total(a.de) : a.de.np;      // floats of the DE's accumulators in LDS (tile-major off the staged path)
    const int ae_at = gg ? 0 : de_acc;                                 // the AE's accumulators in LDS (when !ggA) sit behind the DE's
    const int ae_acc = (AE_TM && !ggA) ? tm_total(a.ae) : a.ae.np;
    const int np_all = ae_at + ((a.dae && !ggA) ? ae_acc : 0);        // floats of LDS accumulators
    float* qb = gacc_l + ((np_all + 3) & ~3);
    const QOff qo = q_offsets(a.de), qoA = q_offsets(a.ae);           // (one region: the two MLPs' evaluations never overlap in time)
    float* upre = u_region(lds, a);                                  // (likewise one region for both MLPs' pre-activations)
    RegFwd rfw;
    RegBwd rbw;
    if constexpr (REG) load_reg_images(a, rfw, rbw);

    auto gb = [&](int c) -> long long { const long long b = b0 + c; return b < a.B ? b : a.B - 1; };
    auto on = [&](int c) -> bool { return b0 + c < a.B; };
    // loops over [rows][TB] tiles: idx -> (r, c)
#define TILE_LOOP(rows) for (int idx = tid, r = tid / TB, c = tid % TB; idx < (rows) * TB; idx += NT, r = idx / TB, c = idx % TB)

    if constexpr (Bd::rk) {      // the tableau -> LDS (coef_a, coef_b)
        static_assert(TP >= 20, "the tableau needs 20 floats of the fourth ks slot (nx = x_dim * TP)");
        if (tid < 20) ks[3 * nx + tid] = tid < 16 ? rk.a[tid >> 2][tid & 3] : rk.b[tid - 16];
    }
    for (int e = tid; e < np_all; e += NT) gacc_l[e] = 0.0f;
    // global accumulators: tile-major slices (tmpart) for the MLPs off the staged path, the natural partial slice itself for a staged one
    float* tmg = a.tmpart + (Bd::par ? wg : (size_t)blockIdx.x) * (tm_total(a.de) + (a.dae ? tm_total(a.ae) : 0));
    float* tmgA = tmg + tm_total(a.de);
    if constexpr (gg) {
        if constexpr (DE_TM) { for (int e = tid; e < tm_total(a.de); e += NT) tmg[e] = 0.0f; }
        else { for (int e = tid; e < a.de.np; e += NT) gacc_g[e] = 0.0f; }
    }
    if constexpr (ggA) {
        if (dae) {
            if constexpr (AE_TM) { for (int e = tid; e < tm_total(a.ae); e += NT) tmgA[e] = 0.0f; }
            else { for (int e = tid; e < a.ae.np; e += NT) gacc_g[a.de.np + e] = 0.0f; }
        }
    }
    TILE_LOOP(n) { a0s[r * TP + c] = a.a0[gb(c) * n + r]; ga0s[r * TP + c] = 0.0f; }
    // (Bd::par: the chunk's last grid point k_hi -- T - 1, or the restart point behind which the sequential sweep holds these two rows alone)
    TILE_LOOP(xd) gxc[r * TP + c] = on(c) ? a.gxs[((Bd::par ? k_hi : a.T - 1) * a.B + gb(c)) * xd + r] : 0.0f;
    TILE_LOOP(id) gic[r * TP + c] = (on(c) && a.gis) ? a.gis[((Bd::par ? k_hi : a.T - 1) * a.B + gb(c)) * id + r] : 0.0f;
    TILE_LOOP(nzv) {   // the last grid point's z|v only receive the AE part (DAE) or nothing (ODE)
        if (!on(c)) continue;
        if constexpr (Bd::par) { if (!last_chunk) continue; }      // (row k_hi of another chunk is chunk c + 1's, written in its step (4))
        const bool isz = r < zd;
        float* dst = isz ? a.gz : a.gv;
        if (dst) dst[((a.T - 1) * a.B + b0 + c) * (isz ? zd : vd) + (isz ? r : r - zd)] = 0.0f;
    }
    if constexpr (Bd::lag) {
        // every row of grad_z / grad_v and every jump gradient starts at zero: a row collects the shares of up to five intervals, each added
        // in (4) by the thread that owns the element here too (idx -> (r, c) is the same in every TILE_LOOP)
        TILE_LOOP(nzv) {
            if (!on(c)) continue;
            const bool isz = r < zd;
            const int d_ = isz ? r : r - zd, w_ = isz ? zd : vd;
            float* dst = isz ? a.gz : a.gv;
            float* dj = isz ? a.gzj : a.gvj;
            if (dst) for (long long j = 0; j < a.T; ++j) dst[(j * a.B + b0 + c) * w_ + d_] = 0.0f;
            if (dj) for (int e = 0; e < a.n_events; ++e) dj[((b0 + c) * a.n_events + e) * w_ + d_] = 0.0f;
        }
    }
    __syncthreads();

    // DE input rows of acts: a0 | s - a0 | s  with s = x | ext
    auto de_input = [&](const float* xs_rows) {
        float* u = acts + a.de.act[0] * TP;
        TILE_LOOP(n) {
            const float s = r < xd ? xs_rows[r * TP + c] : ext[(r - xd) * TP + c];
            const float i0 = a0s[r * TP + c];
            u[r * TP + c] = i0;
            u[(n + r) * TP + c] = s - i0;
            u[(2 * n + r) * TP + c] = s;
        }
        __syncthreads();
    };
    // AE input rows: a0 | x | z | v ; x from xrows (LDS) ; z|v from grid point jzv (>= 0) or from ext
    auto ae_input = [&](const float* xrows, long long jzv) {
        float* u = acts + a.ae.act[0] * TP;
        TILE_LOOP(n + xd + nzv) {
            float v;
            if (r < n) v = a0s[r * TP + c];
            else if (r < n + xd) v = xrows[(r - n) * TP + c];
            else if (jzv < 0) v = ext[(r - n - xd) * TP + c];
            else if (r < n + xd + zd) v = a.z.p[jzv * a.z.st + gb(c) * a.z.sb + (r - n - xd)];
            else v = a.v.p[jzv * a.v.st + gb(c) * a.v.sb + (r - n - xd - zd)];
            u[r * TP + c] = v;
        }
        __syncthreads();
    };
    // VJP of the AE head at (xrows; z|v of grid point jzv or the jumped ext rows) with output gradient `gi`:
    // adds to gx_dst, ga0s, and to the z|v gradients (global gz/gv at jzv, or the jump gradients of event ev; sub-step build, ev == -2: the
    // z | v rows of gext, which collect an interval's sub-steps)
    [[maybe_unused]] float th_head = 0.0f;      // Bd::lin: theta of the in-interval head whose VJP runs (ev == -2)
    auto ae_vjp = [&](const float* xrows, long long jzv, int ev, const float* gi, float* gx_dst) {
        ae_input(xrows, jzv);
        if constexpr (STR >= 1) g_forward_str(a.ae, a.fimgA, acts, qb, qoA, ActCtx{act.ae, upre}); else g_forward(a.ae, acts, wbuf, ActCtx{act.ae, upre});
        TILE_LOOP(id) dA[r * TP + c] = gi[r * TP + c];
        __syncthreads();
        const float* gu = STR >= 1 ? g_vjp_str<ggA>(a.ae, a.timgA, acts, dA, dB, gacc_l + ae_at, tmgA, qb, qoA, ActCtx{act.ae, upre})
                                   : g_vjp<ggA>(a.ae, acts, dA, dB, gacc_l + ae_at, gacc_g + a.de.np, wbuf, ActCtx{act.ae, upre});
        TILE_LOOP(n) ga0s[r * TP + c] += gu[r * TP + c];
        TILE_LOOP(xd) gx_dst[r * TP + c] += gu[(n + r) * TP + c];
        TILE_LOOP(nzv) {
            if (!on(c)) continue;
            const float g = gu[(n + xd + r) * TP + c];
            const bool isz = r < zd;
            const int d_ = isz ? r : r - zd, w_ = isz ? zd : vd;
            if constexpr (Bd::sub) {
                if (ev == -2) {
                    if constexpr (Bd::lag) {
                        const LagW lw = lag_weights(lag_st.off, lag_st.q, th_head);
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            if (m < lag_st.q) gn[(m * nzv + r) * TP + c] += lw.w[m] * g;
                    } else
                    if constexpr (Bd::lin) { gext[r * TP + c] += (1.0f - th_head) * g; gexr[r * TP + c] += th_head * g; }
                    else gext[r * TP + c] += g;
                    continue;
                }
            }
            if constexpr (Bd::pev) { if (jzv < 0 && ev < 0) continue; }      // (the event-time head of a column without a hit: no jump row is its)
            if constexpr (Bd::par) {
                // the head at the chunk's last grid point: row k_hi is chunk c + 1's, which writes it with `=` -- the share goes to this
                // chunk's border slot, and the fold behind the sweep adds it onto the row (the sequential order: step k_hi's value, the
                // restart head's, then this one)
                if (jzv == k_hi && !last_chunk) { msp_border(sub)[((size_t)blockIdx.y * a.B + b0 + c) * nzv + r] = g; continue; }
            }
            if (jzv >= 0) {
                float* dst = isz ? a.gz : a.gv;
                if (dst) dst[(jzv * a.B + b0 + c) * w_ + d_] += g;
            } else {
                float* dst = isz ? a.gzj : a.gvj;
                if (dst) dst[((b0 + c) * a.n_events + ev) * w_ + d_] += g;
            }
        }
        __syncthreads();
    };

    // Look-ahead (round 6): the rows a step reads from HBM -- the clocks, the dataset z | v, xs[k] (x_true[k] under INPUT_TRUE_X), the incoming
    // gradient of grid point k --
    // are requested one step early into registers (items tid + 256 j, j < LA: up to 32 rows each; rows beyond that are loaded where they are
    // used), so that their latency hides behind the previous step instead of standing at the top and the bottom of every step.
    constexpr int LA = 2;
    float la_x[LA], la_g[LA], la_zv[LA], la_t = 0.0f, la_tn = 0.0f;
    auto look_ahead = [&](long long kk) {       // grid point kk >= 0
#pragma unroll
        for (int j = 0; j < LA; ++j) {
            const int idx = tid + NT * j;
            const int ix = idx < xd * TB ? idx : 0, rx = ix / TB, cx = ix % TB;
            la_x[j] = xsrc[(kk * a.B + gb(cx)) * xd + rx];
            la_g[j] = a.gxs[(kk * a.B + gb(cx)) * xd + rx];
            const int iz = idx < nzv * TB ? idx : 0, rz = iz / TB;
            const long long b = gb(iz % TB);
            la_zv[j] = nzv == 0 ? 0.0f : (rz < zd ? a.z.p[kk * a.z.st + b * a.z.sb + rz] : a.v.p[kk * a.v.st + b * a.v.sb + (rz - zd)]);
        }
        if (tid < TB) la_t = a.t.p[kk * a.t.st + gb(tid) * a.t.sb];
    };
    // (the Adams-Bashforth build pins the grid length in scalar registers, as K0's sub-step builds do: left to the compiler the sweep's loop
    //  guard becomes a vector compare, and what it then parks in AGPRs in front of the loop counts as stored under partial EXEC)
    [[maybe_unused]] long long Tu = 0;
    if constexpr (Bd::ab3) Tu = T3;
    else if constexpr (Bd::ab) {
        const unsigned long long u = (unsigned long long)a.T;
        Tu = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)u));
    }
    if constexpr (Bd::par) {
        if (k_hi > k_lo) {
            if (tid < TB) la_tn = a.t.p[k_hi * a.t.st + gb(tid) * a.t.sb];
            look_ahead(k_hi - 1);
        }
    } else {
    if ((Bd::ab ? Tu : a.T) >= 2) {
        if (tid < TB) la_tn = a.t.p[(a.T - 1) * a.t.st + gb(tid) * a.t.sb];
        look_ahead(a.T - 2);
    }
    }
    // Adams-Bashforth 2 (Bd::ab; one stage, one sub-step): the DE's VJP of step k takes phi_k = c0_k g_{k+1} + c1_{k+1} g_{k+2}.  gxc is
    // g_{k+1}; g_{k+2} is kept in gks' slot 1 and the per-column c1_{k+1} in its slot 2 (a one-stage build uses slot 0 alone); c0_k takes h's
    // place in dts.  The threads < TB, which hold the clocks, keep what the coefficients need beyond t[k], t[k+1]: t[k-1] (la_tm, requested
    // one step early like the other look-ahead rows), h_{k+1} (h_n) and step k + 1's event index (ev_n).  K0's expressions, so K0's values.
    // The event table is read through strides: [T - 1][B], or the shared [T - 1] with a column stride of 0; it may be null.
    [[maybe_unused]] long long ev_sk = 1, ev_sb = 0;
    [[maybe_unused]] float la_tm = 0.0f, h_n = 0.0f;
    [[maybe_unused]] int ev_n = -1;
    if constexpr (Bd::ab) {
        if (ev_table_pt(sub)) { ev_sk = a.B; ev_sb = 1; }
        la_tm = a.t.p[(a.T >= 3 ? a.T - 3 : 0) * a.t.st + gb(tid % TB) * a.t.sb];      // (every lane, no branch: see the top of the step; read for k >= 1 only)
    }
    // Adams-Bashforth 3 (Bd::ab3, on Bd::ab's policy): the DE's VJP of step k takes
    //     phi_k = a_k g_{k+1} + c1_{k+1} g_{k+2} + c2_{k+2} g_{k+3} [+ h gamma],   g_k = w_k + g_{k+1} [+ gamma] + (df_k/dx_k)^T phi_k
    // with a_k = h / 2 on a restart step, else c0_k, and gamma the x~ part of the corrector's VJP, run in front of the DE's on a restart step
    // (below, behind (3a)).  g_{k+2} / g_{k+3} live in gks' slots 1 / 3, the per-column a_k, c1_{k+1}, c2_{k+2} and hr = (R_k ? h_k : 0) in
    // dts, gks' slot 2 and ks' slots 0 / 1 (a one-stage build uses neither), x~ and gamma in xst's slots 1 / 2.  Step k computes ITS
    // coefficients with K0's function on K0's values (ab3_coef: t[k-2 .. k+1], the event indices of steps k - 1 and k) and hands c1_k, c2_k
    // on to the next two steps of the sweep in registers of the threads < TB: no forward recurrence.
    [[maybe_unused]] float la_tmm = 0.0f, ab_c1n = 0.0f, ab_c2n = 0.0f, ab_c2nn = 0.0f;
    if constexpr (Bd::ab3) la_tmm = a.t.p[(a.T >= 4 ? a.T - 4 : 0) * a.t.st + gb(tid % TB) * a.t.sb];
    // Multiple shooting (Bd::ms): the step that leaves grid point k > 0 with k % every == 0 started from the dataset row xtr[k] -- and a
    // DAE's DE read the head at that row.  Its stages are recomputed from there; neither its start adjoint nor the x part of that head's VJP
    // travels on.  Launch-uniform: ms_rem is k % every, counted down in a scalar register from one remainder taken in front of the sweep.
    [[maybe_unused]] int ms_w = 0, ms_rem = 0;
    [[maybe_unused]] const float* __restrict__ xtr = nullptr;
    if constexpr (Bd::ms) {
        ms_w = __builtin_amdgcn_readfirstlane(ms_every(sub));
        if constexpr (Bd::par) ms_rem = __builtin_amdgcn_readfirstlane((k_hi > k_lo && ms_w > 0) ? (int)((k_hi - 1) % ms_w) : 0);
        else
        ms_rem = __builtin_amdgcn_readfirstlane((a.T >= 2 && ms_w > 0) ? (int)((a.T - 2) % ms_w) : 0);
        xtr = ms_x_true(sub);
    }
    for (long long k = Bd::par ? k_hi - 1 : (Bd::ab ? Tu : a.T) - 2; k >= (Bd::par ? k_lo : 0); --k) {
        // ev: the event index of this step -- launch-uniform, or (Bd::pev: a [T - 1][B] table, which the host requires) that of this
        // thread's column: every TILE_LOOP and look-ahead item of a thread lies in column tid % TB.  any_ev: some column of the workgroup
        // has a hit (workgroup-uniform: each wave holds every column) -- what decides whether the event-time head is evaluated at all.
        // (the constant conditions on Bd::pev keep the statements of the other builds where they were: their code does not change)
        static_assert(NT % TB == 0 && 64 % TB == 0, "a thread owns one trajectory column, and every wave holds all of them");
        const int ev = Bd::ab ? (a.ev ? a.ev[k * ev_sk + gb(tid % TB) * ev_sb] : -1)
                              : (Bd::pev ? a.ev[k * a.B + gb(tid % TB)] : (a.ev ? a.ev[k] : -1));
        [[maybe_unused]] bool any_ev = false;
        if constexpr (Bd::pev) any_ev = __builtin_amdgcn_ballot_w64(ev >= 0) != 0;
        if constexpr (Bd::ab3) {
            // (as the Adams-Bashforth 2 arm below: every lane runs the arithmetic, the stores are guarded)
            const int ev_m = (a.ev && k >= 1) ? a.ev[(k - 1) * ev_sk + gb(tid % TB) * ev_sb] : -1;      // step k - 1's event, for R_{k-1}
            const float h0 = la_tn - la_t, h1 = la_t - la_tm, h2 = la_tm - la_tmm;                   // h_k, h_{k-1}, h_{k-2}
            const bool rs = k == 0 || ev >= 0 || h1 == 0.0f;
            const bool rp = k <= 1 || ev_m >= 0 || h2 == 0.0f;
            const Ab3Coef cf = ab3_coef(h0, h1, h2, rs, rp || h1 + h2 == 0.0f);
            if (tid < TB) {
                dts[tid] = rs ? h0 * 0.5f : cf.c0;
                gks[2 * nx + tid] = ab_c1n;
                ks[tid] = ab_c2nn;
                ks[nx + tid] = rs ? h0 : 0.0f;
            }
            ab_c2nn = ab_c2n;
            ab_c2n = cf.c2;
            ab_c1n = cf.c1;
            la_tm = la_tmm;
            la_tmm = a.t.p[(k >= 3 ? k - 3 : 0) * a.t.st + gb(tid % TB) * a.t.sb];      // t[(k - 1) - 2], for the next step of the sweep
        } else if constexpr (Bd::ab) {
            // (a thread < TB owns column tid: `ev`, `ev_n` are that column's.  Every lane runs the arithmetic -- the others on zeros, whose
            //  results nobody reads -- and only the stores are guarded: registers that live across steps are then written under full EXEC)
            const float h = la_tn - la_t, hm = la_t - la_tm;      // h_k, h_{k-1} (the latter read for k >= 1 only)
            const bool restart = k == 0 || ev >= 0 || hm == 0.0f;
            const float c0k = restart ? h : h * (1.0f + (h / hm) / 2.0f);
            // c1_{k+1}: absent behind the last step, 0 where step k + 1 restarts (its event, or h_k == 0)
            const bool none = k + 2 > a.T - 1 || ev_n >= 0 || h == 0.0f;
            const float c1n = none ? 0.0f : -(h_n * ((h_n / h) / 2.0f));
            if (tid < TB) { dts[tid] = c0k; gks[2 * nx + tid] = c1n; }
            h_n = h;
            la_tm = a.t.p[(k >= 2 ? k - 2 : 0) * a.t.st + gb(tid % TB) * a.t.sb];      // t[(k - 1) - 1], for the next step of the sweep
            ev_n = ev;
        } else if constexpr (Bd::sub) { if (tid < TB) dts[tid] = Bd::rkc ? la_tn - la_t : (la_tn - la_t) / (float)nsub; }
        else { if (tid < TB) dts[tid] = la_tn - la_t; }
        [[maybe_unused]] bool ms_rs = false;         // (Bd::ms) this step left a restart point
        if constexpr (Bd::ms) {
            ms_rs = ms_rem == 0 && k > 0;
            ms_rem = __builtin_amdgcn_readfirstlane(ms_rem == 0 ? ms_w - 1 : ms_rem - 1);
            if (ms_rs) {      // the look-ahead brought xs[k], the previous segment's prediction: the step started from the dataset row
#pragma unroll
                for (int j = 0; j < LA; ++j) {
                    const int idx = tid + NT * j;
                    const int ix = idx < xd * TB ? idx : 0;
                    la_x[j] = xtr[(k * a.B + gb(ix % TB)) * xd + ix / TB];
                }
            }
        }
        float gx_in[LA];                             // the incoming gradient of grid point k, consumed at the bottom of the step
        [[maybe_unused]] float x_keep[LA];           // sub-step build: xs[k] of the look-ahead, for sub-step 0 (x0 holds the later ones' starts first)
#pragma unroll
        for (int j = 0; j < LA; ++j) {
            const int idx = tid + NT * j;
            gx_in[j] = la_g[j];
            if constexpr (Bd::sub) x_keep[j] = la_x[j];
            if (idx < xd * TB) x0[(idx / TB) * TP + idx % TB] = la_x[j];
            if (idx < nzv * TB && ev < 0) ext[(idx / TB) * TP + idx % TB] = la_zv[j];
        }
        for (int idx = tid + NT * LA; idx < xd * TB; idx += NT) x0[(idx / TB) * TP + idx % TB] = ((Bd::ms && ms_rs) ? xtr : xsrc)[(k * a.B + gb(idx % TB)) * xd + idx / TB];
        TILE_LOOP(nzv) {
            if (ev < 0 && idx < NT * LA) continue;                                      // (came through the look-ahead registers)
            const long long b = gb(c);
            float v;
            if (r < zd) v = ev >= 0 ? a.zj[b * a.zjb + ev * a.zje + r] : a.z.p[k * a.z.st + b * a.z.sb + r];
            else v = ev >= 0 ? a.vj[b * a.vjb + ev * a.vje + (r - zd)] : a.v.p[k * a.v.st + b * a.v.sb + (r - zd)];
            ext[r * TP + c] = v;
        }
        if constexpr (Bd::lag) {      // the stencil of this thread's column and its node rows (0 beyond q)
            lag_st = lag_stencil(lag_table(sub), k, a.T, a.B, gb(tid % TB));
            lag_evs = a.ev ? a.ev[lag_st.s] : -1;
            TILE_LOOP(nzv) {
                const long long b = gb(c);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float v = 0.0f;
                    if (m < lag_st.q) {
                        if (m == 0 && lag_evs >= 0) v = r < zd ? a.zj[b * a.zjb + lag_evs * a.zje + r] : a.vj[b * a.vjb + lag_evs * a.vje + (r - zd)];
                        else v = r < zd ? a.z.p[(lag_st.s + m) * a.z.st + b * a.z.sb + r] : a.v.p[(lag_st.s + m) * a.v.st + b * a.v.sb + (r - zd)];
                    }
                    wn[(m * nzv + r) * TP + c] = v;
                }
            }
        } else
        if constexpr (Bd::lin) {      // (each thread copies the ext values it wrote itself; the right rows are the dataset's, never jumped)
            TILE_LOOP(nzv) {
                const long long b = gb(c);
                wl[r * TP + c] = ext[r * TP + c];
                wr[r * TP + c] = r < zd ? a.z.p[(k + 1) * a.z.st + b * a.z.sb + r] : a.v.p[(k + 1) * a.v.st + b * a.v.sb + (r - zd)];
            }
        }
        if (tid < TB) la_tn = la_t;
        if (k > 0) look_ahead(k - 1);
        __syncthreads();
        // Sub-step nsub - 1 - si.i of the interval, last to first (one pass in the builds without sub-steps).  gxc carries between them; the
        // z | v rows of gext collect all of them before (4); a sub-step behind the first (`inner`) starts from x_sub[k][that - 1], and where
        // the DAE integrates its own i its algebraic input is the head at that state and the interval's z | v.
        SubIter<Bd::sub> si(nsub);
        do {
        const bool inner = !si.last();
        // Bd::lin: theta of stage s of this sub-step, (js + c_s) / nsub with c_s the tableau's row sum in increasing index (wave-uniform), and
        // the z | v rows of ext at it -- the expression K0's stage pass evaluates
        [[maybe_unused]] auto theta = [&](int s) -> float {
            float cs = 0.0f;
            for (int j = 0; j < s; ++j) cs += coef_a(a.method, ks, nx, s, j);
            return rk_u(((float)(nsub - 1 - si.i) + cs) / (float)nsub);
        };
        [[maybe_unused]] auto lin_ext = [&](float th) {      // (no barrier of its own)
            if constexpr (Bd::lag) {      // K0's weights and K0's sum (lag_weights, lag_eval)
                const LagW lw = lag_weights(lag_st.off, lag_st.q, th);
                TILE_LOOP(nzv) ext[r * TP + c] = lag_eval(lw, lag_st.q, wn[r * TP + c], wn[(nzv + r) * TP + c], wn[(2 * nzv + r) * TP + c], wn[(3 * nzv + r) * TP + c]);
            } else {
            TILE_LOOP(nzv) { const float l_ = wl[r * TP + c]; ext[r * TP + c] = l_ + th * (wr[r * TP + c] - l_); }
            }
        };
        if constexpr (Bd::sub) {
            if (nsub > 1) {      // (defensive: the host never launches this build with one sub-step -- substeps == 1 takes the other entry points)
                const int js = nsub - 1 - si.i;
                if (js > 0) {
                    TILE_LOOP(xd) x0[r * TP + c] = sub.x_sub[((k * (nsub - 1) + js - 1) * a.B + gb(c)) * xd + r];
                } else {      // back to xs[k]: from the look-ahead registers, rows beyond them from memory as at the top of the step
#pragma unroll
                    for (int j = 0; j < LA; ++j) {
                        const int idx = tid + NT * j;
                        if (idx < xd * TB) x0[(idx / TB) * TP + idx % TB] = x_keep[j];
                    }
                    for (int idx = tid + NT * LA; idx < xd * TB; idx += NT) x0[(idx / TB) * TP + idx % TB] = ((Bd::ms && ms_rs) ? xtr : xsrc)[(k * a.B + gb(idx % TB)) * xd + idx / TB];
                }
                if constexpr (Bd::lin) lin_ext(theta(0));      // what the head in front of this sub-step (or the event's) saw
                __syncthreads();
            }
        }
        if (dae) {
            // (1) AE head at the end of step k: i_{k+1} = g(x_{k+1}; z[k+1], v[k+1]) carries gic
            //     (tx: the head read x_true[k+1] and its x-adjoint is dropped -- gx0 is rewritten in (3b))
            if (si.first()) {
            TILE_LOOP(xd) xst[r * TP + c] = xsrc[((k + 1) * a.B + gb(c)) * xd + r];
            __syncthreads();
            ae_vjp(xst, k + 1, -1, gic, tx ? gx0 : gxc);
            }
            // (2) algebraic input of this step's DE (ti: the dataset row, also on event steps)
            if (ti) {
                TILE_LOOP(id) ext[(nzv + r) * TP + c] = a.it[(k * a.B + gb(c)) * id + r];
            } else if ((Bd::pev ? any_ev : (ev >= 0 || (Bd::ms && ms_rs))) || inner) {      // (a restart's head: x0 is the dataset row, ext's z | v rows those of grid point k or the jumped ones)
                const float* xr = x0;
                if (tx && !inner) {       // the event-time head reads the RUNNING state xs[k], not the row the DE starts from (xst is free until (3a))
                    TILE_LOOP(xd) xst[r * TP + c] = a.xs[(k * a.B + gb(c)) * xd + r];
                    __syncthreads();
                    xr = xst;
                }
                ae_input(xr, -1);
                if constexpr (STR >= 1) g_forward_str(a.ae, a.fimgA, acts, qb, qoA, ActCtx{act.ae, upre}); else g_forward(a.ae, acts, wbuf, ActCtx{act.ae, upre});
                const float* out = acts + a.ae.act[a.ae.L] * TP;
                if constexpr (Bd::pev) {      // the event-time head is taken by the columns with a hit; the others read the i they carried
                    TILE_LOOP(id) ext[(nzv + r) * TP + c] = (inner || ev >= 0) ? out[r * TP + c] : a.is_[(k * a.B + gb(c)) * id + r];
                } else {
                    TILE_LOOP(id) ext[(nzv + r) * TP + c] = out[r * TP + c];
                }
            } else {
                TILE_LOOP(id) ext[(nzv + r) * TP + c] = a.is_[(k * a.B + gb(c)) * id + r];
            }
            if constexpr (Bd::sth) { if (sth_on) { TILE_LOOP(id) gic[r * TP + c] = ext[(nzv + r) * TP + c]; } }      // stage 0's i (each thread copies what it wrote)
            __syncthreads();
        }
        // (3a) stage inputs and slopes
        for (int s = 0; s < S; ++s) {
            TILE_LOOP(xd) {
                float acc = 0.0f;
                for (int j = 0; j < s; ++j) {      // (the tableau build skips a coefficient that is exactly 0)
                    const float cf = coef_a(a.method, ks, nx, s, j);
                    if constexpr (Bd::rk) { if (cf != 0.0f) acc += cf * ks[j * nx + r * TP + c]; } else acc += cf * ks[j * nx + r * TP + c];
                }
                xst[s * nx + r * TP + c] = s == 0 ? x0[r * TP + c] : x0[r * TP + c] + dts[c] * acc;
            }
            if constexpr (Bd::lin) lin_ext(theta(s));      // (behind the loop ext holds the last stage's rows, (3b)'s first)
            __syncthreads();
            if constexpr (Bd::sth) {
                if (sth_on && s > 0) {      // i_s = g(X_s; z | v at theta_s), K0's evaluation between the stages s - 1 and s
                    ae_input(xst + s * nx, -1);
                    if constexpr (STR >= 1) g_forward_str(a.ae, a.fimgA, acts, qb, qoA, ActCtx{act.ae, upre}); else g_forward(a.ae, acts, wbuf, ActCtx{act.ae, upre});
                    const float* out = acts + a.ae.act[a.ae.L] * TP;
                    TILE_LOOP(id) ext[(nzv + r) * TP + c] = out[r * TP + c];
                    __syncthreads();
                }
            }
            if (s + 1 < S) {               // (the last stage's slope feeds no stage input: its evaluation is (3b)'s first, not done here)
                de_input(xst + s * nx);
                if constexpr (REG) g_forward_reg(a, acts, qb, qo, rfw, ActCtx{act.de, upre});
                else if constexpr (STR == 2) g_forward_str(a.de, a.fimg, acts, qb, qo, ActCtx{act.de, upre});
                else g_forward(a.de, acts, wbuf, ActCtx{act.de, upre});
                const float* out = acts + a.de.act[a.de.L] * TP;
                TILE_LOOP(xd) ks[s * nx + r * TP + c] = out[r * TP + c];
                __syncthreads();
            }
        }
        // (Bd::ab3) The corrector's VJP, where some column of the workgroup restarts with h != 0 (workgroup-uniform: each wave holds every
        // column; a restart with h == 0 feeds it a zero cotangent).  f_k and x~ = x_k + h f_k are recomputed, then i~ = AE(x~; rows k + 1)
        // for a DAE, then the DE at (x~; rows k + 1, i~) with the cotangent (h / 2) g_{k+1} -- zero in the columns that do not restart, so
        // that they add nothing anywhere.  Its z | v part is ADDED to row k + 1 of grad_z / grad_v by the thread that wrote that row one
        // step earlier (the last row: zeroed up front) and that alone has added to it since; the algebraic part goes through the head at
        // x~; the x~ parts of both are gamma.  gext keeps the step's ext rows meanwhile, gic (free between (1) and (4)) i~'s adjoint.
        if constexpr (Bd::ab3) {
            if (__builtin_amdgcn_ballot_w64(ks[nx + tid % TB] != 0.0f) != 0) {
                float* xp = xst + nx;          // x~
                float* gam = xst + 2 * nx;     // gamma
                de_input(xst);
                if constexpr (REG) g_forward_reg(a, acts, qb, qo, rfw, ActCtx{act.de, upre});
                else if constexpr (STR == 2) g_forward_str(a.de, a.fimg, acts, qb, qo, ActCtx{act.de, upre});
                else g_forward(a.de, acts, wbuf, ActCtx{act.de, upre});
                {
                    const float* out = acts + a.de.act[a.de.L] * TP;
                    TILE_LOOP(xd) xp[r * TP + c] = x0[r * TP + c] + ks[nx + c] * out[r * TP + c];
                }
                TILE_LOOP(ne) gext[r * TP + c] = ext[r * TP + c];
                TILE_LOOP(nzv) {
                    const long long b = gb(c);
                    ext[r * TP + c] = r < zd ? a.z.p[(k + 1) * a.z.st + b * a.z.sb + r] : a.v.p[(k + 1) * a.v.st + b * a.v.sb + (r - zd)];
                }
                __syncthreads();
                if (dae) {
                    ae_input(xp, k + 1);
                    if constexpr (STR >= 1) g_forward_str(a.ae, a.fimgA, acts, qb, qoA, ActCtx{act.ae, upre}); else g_forward(a.ae, acts, wbuf, ActCtx{act.ae, upre});
                    const float* out = acts + a.ae.act[a.ae.L] * TP;
                    TILE_LOOP(id) ext[(nzv + r) * TP + c] = out[r * TP + c];
                    __syncthreads();
                }
                de_input(xp);
                if constexpr (REG) g_forward_reg(a, acts, qb, qo, rfw, ActCtx{act.de, upre});
                else if constexpr (STR == 2) g_forward_str(a.de, a.fimg, acts, qb, qo, ActCtx{act.de, upre});
                else g_forward(a.de, acts, wbuf, ActCtx{act.de, upre});
                TILE_LOOP(xd) dA[r * TP + c] = (ks[nx + c] * 0.5f) * gxc[r * TP + c];
                __syncthreads();
                const float* gu = REG ? g_vjp_reg<gg>(a, acts, dA, dB, gacc_l, tmg, qb, qo, rbw, ActCtx{act.de, upre})
                                      : (STR == 2 ? g_vjp_str<gg>(a.de, a.timg, acts, dA, dB, gacc_l, tmg, qb, qo, ActCtx{act.de, upre})
                                                  : g_vjp<gg>(a.de, acts, dA, dB, gacc_l, gacc_g, wbuf, ActCtx{act.de, upre}));
                TILE_LOOP(n) {      // (ext's corrector rows are spent: it stages their adjoints for the threads that own the rows)
                    const float gs = gu[(n + r) * TP + c] + gu[(2 * n + r) * TP + c];
                    ga0s[r * TP + c] += gu[r * TP + c] - gu[(n + r) * TP + c];
                    if (r < xd) gam[r * TP + c] = gs; else ext[(r - xd) * TP + c] = gs;
                }
                __syncthreads();
                TILE_LOOP(nzv) {
                    if (!on(c)) continue;
                    const bool isz = r < zd;
                    float* dst = isz ? a.gz : a.gv;
                    if (dst) dst[((k + 1) * a.B + b0 + c) * (isz ? zd : vd) + (isz ? r : r - zd)] += ext[r * TP + c];
                }
                TILE_LOOP(id) gic[r * TP + c] = ext[(nzv + r) * TP + c];
                __syncthreads();
                if (dae) ae_vjp(xp, k + 1, -1, gic, gam);
                TILE_LOOP(ne) ext[r * TP + c] = gext[r * TP + c];
                __syncthreads();
            }
        }
        // (3b) stages backwards
        TILE_LOOP(xd) {
            const float g1 = gxc[r * TP + c];
            gx0[r * TP + c] = g1;
            if constexpr (Bd::ab3) {      // phi_k; the history's slots are unwritten at the first steps of the sweep, where c1 / c2 are 0
                const float c1n = gks[2 * nx + c], c2nn = ks[c], hr = ks[nx + c];
                float phi = dts[c] * g1;
                if (c1n != 0.0f) phi = phi + c1n * gks[nx + r * TP + c];
                if (c2nn != 0.0f) phi = phi + c2nn * gks[3 * nx + r * TP + c];
                if (hr != 0.0f) {
                    const float gm = xst[2 * nx + r * TP + c];
                    phi = phi + hr * gm;
                    gx0[r * TP + c] = g1 + gm;
                }
                gks[r * TP + c] = phi;
                gks[3 * nx + r * TP + c] = gks[nx + r * TP + c];      // g_{k+2} -> g_{k+3}, g_{k+1} -> g_{k+2} for step k - 1: this thread's alone
                gks[nx + r * TP + c] = g1;
            } else if constexpr (Bd::rkc) {
                // Runge-Kutta-Chebyshev (Bd::rkc; one stage per pass, nsub = the stage count): this pass is stage j = nsub - si.i, g1 the adjoint
                // lam of Y_j.  The DE's VJP at Y_{j-1} takes (mut_j h) lam, at j = 1 plus the adjoint of F_0; gx0, the adjoint of Y_{j-1}, starts
                // from what the later stages left it (nu_{j+1} lam_{j+1}, in gks' slot 1) plus mu_j lam, and the VJP and the head add to it; slot 1
                // then takes nu_j lam for Y_{j-2}, slots 2 / 3 collect the adjoints of Y_0 (kap_j lam) and F_0 ((gam_j h) lam).  Stage 1's Y_{j-1}
                // is Y_0: its adjoint takes slot 2 and lam.  The slots are unwritten in front of the interval's first pass, which reads none.
                const RkcCoef rc = rkc_coef(sub, nsub - 1 - si.i);
                const bool top = si.first();
                const float pj = top ? 0.0f : gks[nx + r * TP + c], gy0 = top ? 0.0f : gks[2 * nx + r * TP + c], gf0 = top ? 0.0f : gks[3 * nx + r * TP + c];
                const float hl = (rc.mut * dts[c]) * g1;
                if (!si.last()) {
                    gks[r * TP + c] = hl;
                    gx0[r * TP + c] = pj + rc.mu * g1;
                    gks[nx + r * TP + c] = rc.nu * g1;
                    gks[2 * nx + r * TP + c] = gy0 + rc.kap * g1;
                    gks[3 * nx + r * TP + c] = gf0 + (rc.gam * dts[c]) * g1;
                } else {
                    gks[r * TP + c] = hl + gf0;
                    gx0[r * TP + c] = (pj + gy0) + g1;
                }
            } else if constexpr (Bd::ab) {      // phi_k; g_{k+2}'s slot is unwritten at the first step of the sweep, where c1 is 0
                const float c1n = gks[2 * nx + c];
                float phi = dts[c] * g1;
                if (c1n != 0.0f) phi = phi + c1n * gks[nx + r * TP + c];
                gks[r * TP + c] = phi;
                gks[nx + r * TP + c] = g1;      // g_{k+1} for step k - 1: written and read by this thread alone
            } else {
            for (int s = 0; s < S; ++s) gks[s * nx + r * TP + c] = dts[c] * coef_b(a.method, ks, nx, s) * g1;
            }
        }
        if constexpr (Bd::lag) {
            if (si.first()) { TILE_LOOP(nzv) { gn[r * TP + c] = 0.0f; gn[(nzv + r) * TP + c] = 0.0f; gn[(2 * nzv + r) * TP + c] = 0.0f; gn[(3 * nzv + r) * TP + c] = 0.0f; } }
        } else
        if constexpr (Bd::lin) { if (si.first()) { TILE_LOOP(nzv) gexr[r * TP + c] = 0.0f; } }
        if constexpr (Bd::sub) { TILE_LOOP(ne) if (r >= nzv || si.first()) gext[r * TP + c] = 0.0f; }
        else { TILE_LOOP(ne) gext[r * TP + c] = 0.0f; }
        __syncthreads();
        for (int s = S - 1; s >= 0; --s) {
            de_input(xst + s * nx);
            if constexpr (REG) { if (PSNODE_K5_ABL != 3) g_forward_reg(a, acts, qb, qo, rfw, ActCtx{act.de, upre}); }
            else if constexpr (STR == 2) g_forward_str(a.de, a.fimg, acts, qb, qo, ActCtx{act.de, upre});
            else g_forward(a.de, acts, wbuf, ActCtx{act.de, upre});
            TILE_LOOP(xd) dA[r * TP + c] = gks[s * nx + r * TP + c];
            __syncthreads();
            const float* gu = REG ? g_vjp_reg<gg>(a, acts, dA, dB, gacc_l, tmg, qb, qo, rbw, ActCtx{act.de, upre})
                                  : (STR == 2 ? g_vjp_str<gg>(a.de, a.timg, acts, dA, dB, gacc_l, tmg, qb, qo, ActCtx{act.de, upre})
                                              : g_vjp<gg>(a.de, acts, dA, dB, gacc_l, gacc_g, wbuf, ActCtx{act.de, upre}));
            [[maybe_unused]] float th_s = 0.0f;
            if constexpr (Bd::lin) th_s = theta(s);
            [[maybe_unused]] LagW lw_s{};
            if constexpr (Bd::lag) lw_s = lag_weights(lag_st.off, lag_st.q, th_s);
            TILE_LOOP(n) {
                const float gs = gu[(n + r) * TP + c] + gu[(2 * n + r) * TP + c];
                ga0s[r * TP + c] += gu[r * TP + c] - gu[(n + r) * TP + c];
                if (r < xd) {
                    gx0[r * TP + c] += gs;
                    for (int j = 0; j < s; ++j) {
                        if constexpr (Bd::rk) { const float cf = coef_a(a.method, ks, nx, s, j); if (cf != 0.0f) gks[j * nx + r * TP + c] += dts[c] * cf * gs; }
                        else gks[j * nx + r * TP + c] += dts[c] * coef_a(a.method, ks, nx, s, j) * gs;
                    }
                } else {
                    if constexpr (Bd::lag) {
                        if (r - xd < nzv) {      // w = sum_m l_m(u) node_m: the stage's external adjoint goes to the q nodes
#pragma unroll
                            for (int m = 0; m < 4; ++m)
                                if (m < lag_st.q) gn[(m * nzv + r - xd) * TP + c] += lw_s.w[m] * gs;
                        } else {
                            gext[(r - xd) * TP + c] += gs;
                        }
                    } else
                    if constexpr (Bd::lin) {
                        if (r - xd < nzv) {      // w = w_L + theta (w_R - w_L): the stage's external adjoint goes to both ends
                            gext[(r - xd) * TP + c] += (1.0f - th_s) * gs;
                            gexr[(r - xd) * TP + c] += th_s * gs;
                        } else {
                            gext[(r - xd) * TP + c] += gs;
                        }
                    } else {
                        gext[(r - xd) * TP + c] += gs;
                    }
                }
            }
            if constexpr (Bd::sth) {
                if (sth_on && s > 0) {
                    // gext's i rows hold stage s's algebraic adjoint alone: through the head at (X_s; ext's rows, still theta_s's)
                    TILE_LOOP(xd) gxc[r * TP + c] = 0.0f;
                    __syncthreads();
                    th_head = theta(s);
                    ae_vjp(xst + s * nx, -1, -2, gext + nzv * TP, gxc);
                    TILE_LOOP(xd) {      // the x part is one more share of X_s's adjoint: onto the start state and over k_j by a[s][j]
                        const float g = gxc[r * TP + c];
                        gx0[r * TP + c] += g;
                        for (int j = 0; j < s; ++j) { const float cf = coef_a(a.method, ks, nx, s, j); if (cf != 0.0f) gks[j * nx + r * TP + c] += dts[c] * cf * g; }
                    }
                    TILE_LOOP(id) gext[(nzv + r) * TP + c] = 0.0f;
                    lin_ext(theta(s - 1));
                    __syncthreads();
                    if (s > 1) {      // stage s - 1's algebraic input, recomputed
                        ae_input(xst + (s - 1) * nx, -1);
                        if constexpr (STR >= 1) g_forward_str(a.ae, a.fimgA, acts, qb, qoA, ActCtx{act.ae, upre}); else g_forward(a.ae, acts, wbuf, ActCtx{act.ae, upre});
                        const float* out = acts + a.ae.act[a.ae.L] * TP;
                        TILE_LOOP(id) ext[(nzv + r) * TP + c] = out[r * TP + c];
                    } else {
                        TILE_LOOP(id) ext[(nzv + r) * TP + c] = gic[r * TP + c];
                    }
                    __syncthreads();
                    continue;
                }
            }
            if constexpr (Bd::lin) { if (s > 0) lin_ext(theta(s - 1)); }      // (ext was copied into the DE input before the VJP)
            __syncthreads();
        }
        if constexpr (Bd::sub) {
            if (inner) {      // the head that fed this sub-step's DE: into its start state's adjoint, ga0s and the interval's z | v
                if constexpr (Bd::lin) th_head = theta(0);
                if (dae && !ti) ae_vjp(x0, -1, -2, gext + nzv * TP, gx0);
                TILE_LOOP(xd) gxc[r * TP + c] = gx0[r * TP + c];
                __syncthreads();
                continue;
            }
        }
        // tx: the step started from a dataset row -- its start adjoint goes nowhere (an ODE keeps step 0's: grad_x0 = grad_xs[0] + it), and
        // gx0 from here on collects what still reaches the running state xs[k]: the event-time head's x-adjoint
        if (tx && (dae || k > 0)) { TILE_LOOP(xd) gx0[r * TP + c] = 0.0f; }
        if constexpr (Bd::ms) { if (ms_rs) { TILE_LOOP(xd) gx0[r * TP + c] = 0.0f; } }      // (likewise: gxc becomes gxs[k] alone)
        // (4) gradients of this step's external inputs
        TILE_LOOP(nzv) {
            if (!on(c)) continue;
            const float g = gext[r * TP + c];
            const bool isz = r < zd;
            const int d_ = isz ? r : r - zd, w_ = isz ? zd : vd;
            float* dst = isz ? a.gz : a.gv;
            float* dj = isz ? a.gzj : a.gvj;
            if constexpr (Bd::lag) {
                // node m's sum: ADDED to row s + m -- zeroed up front, this thread's alone -- or, for a jumped node s, to the jump gradient of
                // the event at step s (gext's z | v rows stay zero in this build)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (m >= lag_st.q) continue;
                    const float gm = gn[(m * nzv + r) * TP + c];
                    if (m == 0 && lag_evs >= 0) { if (dj) dj[((b0 + c) * a.n_events + lag_evs) * w_ + d_] += gm; }
                    else if (dst) dst[((lag_st.s + m) * a.B + b0 + c) * w_ + d_] += gm;
                }
                continue;
            }
            if (ev >= 0) {
                if (dj) dj[((b0 + c) * a.n_events + ev) * w_ + d_] = g;
                if (dst) dst[(k * a.B + b0 + c) * w_ + d_] = 0.0f;
            } else if (dst) {
                dst[(k * a.B + b0 + c) * w_ + d_] = g;
            }
            // the right sums: into row k + 1, which this thread wrote one interval earlier (the last row: zeroed up front) and to which it
            // alone has added since (the head VJP at grid point k + 1)
            if constexpr (Bd::lin) { if (dst) dst[((k + 1) * a.B + b0 + c) * w_ + d_] += gexr[r * TP + c]; }
        }
        if (dae) {
            __syncthreads();
            if (ti) {        // the DE read i_true[k]: nothing flows back through the algebraic variable
                TILE_LOOP(id) gic[r * TP + c] = (on(c) && a.gis) ? a.gis[(k * a.B + gb(c)) * id + r] : 0.0f;
            } else if (Bd::pev ? any_ev : (ev >= 0 || (Bd::ms && ms_rs))) {   // i_in = g(x_k; jumps): its gradient flows into x_k and the jump inputs; i_k itself was unused
                if constexpr (Bd::pev) {
                    // ... in the columns with a hit.  The others fed the DE the i they carried: their adjoint goes on into gic (the arm
                    // below), and their output gradient is ZERO in the head's VJP, so that they add nothing to its weight gradients, to
                    // ga0s, to gx0 or to a jump row.  (Each thread rewrites the gext elements it reads; ae_vjp's first barrier orders the rest.)
                    TILE_LOOP(id) {
                        const float g = gext[(nzv + r) * TP + c];
                        gic[r * TP + c] = (ev >= 0 ? 0.0f : g) + ((on(c) && a.gis) ? a.gis[(k * a.B + gb(c)) * id + r] : 0.0f);
                        if (ev < 0) gext[(nzv + r) * TP + c] = 0.0f;
                    }
                }
                const float* xr = x0;
                if (tx) {    // (the stages are done with xst)
                    TILE_LOOP(xd) xst[r * TP + c] = a.xs[(k * a.B + gb(c)) * xd + r];
                    __syncthreads();
                    xr = xst;
                }
                if constexpr (Bd::ms) {
                    // a restart's head read the dataset row: the x part of its VJP is discarded.  ae_vjp ADDS it to its destination, so it
                    // is given xst's slot 0 as a sink: the stages are done with xst, which holds this step's stage inputs (finite), and (1) /
                    // (3a) of the next step rewrite every element before anything reads it.  Without an event its z | v rows are grid point k's, whose gradient rows this thread wrote in (4): the event
                    // arm's ordering.
                    ae_vjp(xr, (ms_rs && ev < 0) ? k : -1, ev, gext + nzv * TP, ms_rs ? xst : gx0);
                } else {
                ae_vjp(xr, -1, ev, gext + nzv * TP, gx0);
                }
                if constexpr (!Bd::pev) { TILE_LOOP(id) gic[r * TP + c] = (on(c) && a.gis) ? a.gis[(k * a.B + gb(c)) * id + r] : 0.0f; }
            } else {
                TILE_LOOP(id) gic[r * TP + c] = gext[(nzv + r) * TP + c] + ((on(c) && a.gis) ? a.gis[(k * a.B + gb(c)) * id + r] : 0.0f);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LA; ++j) {
            const int idx = tid + NT * j;
            if (idx < xd * TB) gxc[(idx / TB) * TP + idx % TB] = gx0[(idx / TB) * TP + idx % TB] + (on(idx % TB) ? gx_in[j] : 0.0f);
        }
        for (int idx = tid + NT * LA; idx < xd * TB; idx += NT) {
            const int r = idx / TB, c = idx % TB;
            gxc[r * TP + c] = gx0[r * TP + c] + (on(c) ? a.gxs[(k * a.B + gb(c)) * xd + r] : 0.0f);
        }
        __syncthreads();
        } while (si.more());
    }
    if (dae && !(Bd::par && k_lo > 0)) {   // i_0 = g(x_0; z[0], v[0])   (my_solvers.py:95)
        TILE_LOOP(xd) x0[r * TP + c] = xsrc[gb(c) * xd + r];
        __syncthreads();
        ae_vjp(x0, 0, -1, gic, tx ? gx0 : gxc);
    }
    if constexpr (Bd::par) {      // chunk 0 alone reaches grid point 0; a later chunk leaves its grad_all_initial partial for the fold
        if (k_lo > 0) {
            float* gp = msp_ga0_part(sub) + (size_t)(blockIdx.y - 1) * a.B * n;
            TILE_LOOP(n) if (on(c)) gp[(b0 + c) * n + r] = ga0s[r * TP + c];
        } else {
            TILE_LOOP(xd) if (on(c)) a.gx0[(b0 + c) * xd + r] = gxc[r * TP + c];
            TILE_LOOP(n) if (on(c)) a.ga0[(b0 + c) * n + r] = ga0s[r * TP + c];
        }
    } else {
    TILE_LOOP(xd) if (on(c)) a.gx0[(b0 + c) * xd + r] = gxc[r * TP + c];
    TILE_LOOP(n) if (on(c)) a.ga0[(b0 + c) * n + r] = ga0s[r * TP + c];
    }
    float* wp = a.wpart + (Bd::par ? wg : (size_t)blockIdx.x) * (a.de.np + (dae ? a.ae.np : 0));
    // the LDS accumulators -> this workgroup's partial in nn.Linear order (tile-major ones un-permuted)
    // (volatile: the global tile-major slices were written by other lanes of this workgroup; read them past the vector L1)
    auto unpermute = [&](const GMlp& m, const volatile float* base, float* dst) {
        for (int l = 0; l < m.L; ++l) {
            const int N = m.out_dim[l], K = l ? m.out_dim[l - 1] : m.in_dim, ntk = (K + 15) / 16;
            const volatile float* tw = base + tm_dw_off(m, l);
            for (int e = tid; e < N * K; e += NT) {
                const int j = e / K, k = e % K;
                dst[m.gw[l] + e] = tw[(((j >> 4) * ntk + (k >> 4)) * 64 + ((j & 15) >> 2) * 16 + (k & 15)) * 4 + (j & 3)];
            }
            for (int e = tid; e < N; e += NT) dst[m.gb[l] + e] = base[tm_db_off(m, l) + e];
        }
    };
    if constexpr (!ggA) {
        if (dae) {
            if constexpr (AE_TM) unpermute(a.ae, gacc_l + ae_at, wp + a.de.np);
            else for (int e = tid; e < a.ae.np; e += NT) wp[a.de.np + e] = gacc_l[ae_at + e];
        }
    }
    if constexpr (!gg) {
        if constexpr (DE_TM) unpermute(a.de, gacc_l, wp);
        else for (int e = tid; e < a.de.np; e += NT) wp[e] = gacc_l[e];
    }
    if constexpr (gg && DE_TM) { __threadfence(); __syncthreads(); unpermute(a.de, tmg, wp); }
    if constexpr (ggA && AE_TM) { if (dae) { __threadfence(); __syncthreads(); unpermute(a.ae, tmgA, wp + a.de.np); } }
#undef TILE_LOOP
