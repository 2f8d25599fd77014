// The chain wave's tile machinery of K4f (psnode_backward_fused.hip) and K7f (psnode_dae_backward_fused.hip), as text (the idiom of
// psnode_generic_body.h): each kernel includes this file once in its body, behind its prologue.  As text and not as a struct
// because these kernels sit on the register limit at 8 waves: with the state in a device struct 27 of them spilled more and the DAE
// hidden-128 training step lost 1-5 % (profiles/tile_bwd_toolkit_ab.txt); the closures below compile to the code of the copies they replace.
// In scope: template parameters NWV, REC, ROLES; S (stages); `Tune` (K4fTune / K7fTune: all that differs between the two kernels);
// xb ([2][NWV] exchange tiles), wT (H->H images in LDS, [layer][chunk][wave][lane] f4), scr (this wave's private tile), l, w, g, i.
// Defines: toff, roff, tile, put, getl, get_row, transpose; the exchange parity p; mid, mid_lds, mid_g, dw_groups, flush,
// midT, own4, allreduce2, allreduce4 and the deferral state pendT / pend_h / pend_par.
// (Accumulator chains start from the literal zero, not from a captured constant: the capture moves the register allocation of K4f's
//  two-role Euler / Midpoint instances.)
    static_assert(std::is_same_v<decltype(xb), float*> && std::is_same_v<decltype(scr), float*> && std::is_same_v<decltype(wT), f4*>,
                  "psnode_tile_bwd_chain.h: xb, scr (float*) and wT (f4*) of the including kernel");
    constexpr int BMODE = Tune::bound(REC), EVERY = Tune::every(REC);
    constexpr bool BOUND = NWV >= 8 && (BMODE == 1 || (BMODE == 2 && S >= 4) || (BMODE == 3 && S >= 2));
    // ---- LDS tiles
    const int toff = 4 * l + 8 * g;                                   // own slot of a tile
    const int roff = 72 * (i >> 2) + 4 * g + (i & 3);                 // row i of a tile, columns g, g+4, g+8, g+12
    auto tile = [&](const int par, const int wv) -> float* { return xb + (par * NWV + wv) * FTILE; };
    auto put = [&](float* t_, const f4 v) { *reinterpret_cast<f4*>(t_ + toff) = v; };
    auto getl = [&](const float* t_) -> f4 { return *reinterpret_cast<const f4*>(t_ + toff); };
    auto get_row = [&](const float* t_, const int ro) -> f4 { const float* s_ = t_ + ro; return f4{s_[0], s_[16], s_[32], s_[48]}; };
    auto transpose = [&](const f4 v) -> f4 { put(scr, v); return get_row(scr, roff); };   // own D tile -> operand layout (trajectory g + 4kk)

    int p = 0;
    constexpr bool PREFETCH_ALL = NWV <= 4;
    // forward H->H layer, weights in registers (K1's `mid`); returns the pre-activation
    auto mid = [&](const float (&wm)[4 * NWV], const f4 bias, const f4 h) -> f4 {
        put(tile(p, w), h);
        f4 accA = bias, accB = f4{0.f, 0.f, 0.f, 0.f};
        accA = fm4(wm[0], h[0], accA); accB = fm4(wm[1], h[1], accB);
        accA = fm4(wm[2], h[2], accA); accB = fm4(wm[3], h[3], accB);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
        f4 vq[NWV];
        if constexpr (PREFETCH_ALL) {
#pragma unroll
            for (int c = 1; c < NWV; ++c) vq[c] = getl(tile(p, (w + c) & (NWV - 1)));
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int c = 1; c < NWV; ++c) {
            const f4 v = PREFETCH_ALL ? vq[c] : getl(tile(p, (w + c) & (NWV - 1)));
            accA = fm4(wm[4 * c + 0], v[0], accA); accB = fm4(wm[4 * c + 1], v[1], accB);
            accA = fm4(wm[4 * c + 2], v[2], accA); accB = fm4(wm[4 * c + 3], v[3], accB);
        }
        p ^= 1;
        return accA + accB;
    };
    // H->H layer with image `layer` of wT (forward image: pre-activation from `bias`; transposed image: sum_k W[k][own] d[k])
    auto mid_lds = [&](const int layer, const f4 bias, const f4 h) -> f4 {
        put(tile(p, w), h);
        const f4* wl = Tune::template image<NWV>(wT, layer, w, l);
        f4 wq = wl[0];
        f4 accA = bias, accB = f4{0.f, 0.f, 0.f, 0.f};
        accA = fm4(wq[0], h[0], accA); accB = fm4(wq[1], h[1], accB);
        accA = fm4(wq[2], h[2], accA); accB = fm4(wq[3], h[3], accB);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
#pragma unroll
        for (int c = 1; c < NWV; ++c) {
            const f4 v = getl(tile(p, (w + c) & (NWV - 1)));
            wq = wl[c * NWV * 64];
            accA = fm4(wq[0], v[0], accA); accB = fm4(wq[1], v[1], accB);
            accA = fm4(wq[2], v[2], accA); accB = fm4(wq[3], v[3], accB);
            if constexpr (BOUND) { if (c % EVERY == EVERY - 1) __builtin_amdgcn_sched_barrier(0); }
        }
        p ^= 1;
        return accA + accB;
    };
    // the same with the image read from a packed tensor in global memory (8 waves: the AE's images; the LDS holds the DE's): all chunks
    // are requested before the exchange so that their latency overlaps it
    auto mid_g = [&](const f4* __restrict__ img, const f4 bias, const f4 h) -> f4 {
        const f4* wlo = img + w * 64 + l;
        asm volatile("" : "+v"(wlo));      // opaque: the loads are loop-invariant and would be hoisted out of the time loop (and spilled)
        const gptr<const f4> wl = (gptr<const f4>)wlo;
        f4 wq[NWV];
#pragma unroll
        for (int c = 0; c < NWV; ++c) wq[c] = wl[c * NWV * 64];
        put(tile(p, w), h);
        f4 accA = bias, accB = f4{0.f, 0.f, 0.f, 0.f};
        accA = fm4(wq[0][0], h[0], accA); accB = fm4(wq[0][1], h[1], accB);
        accA = fm4(wq[0][2], h[2], accA); accB = fm4(wq[0][3], h[3], accB);
        lds_barrier();
#pragma unroll
        for (int c = 1; c < NWV; ++c) {
            const f4 v = getl(tile(p, (w + c) & (NWV - 1)));
            accA = fm4(wq[c][0], v[0], accA); accB = fm4(wq[c][1], v[1], accB);
            accA = fm4(wq[c][2], v[2], accA); accB = fm4(wq[c][3], v[3], accB);
        }
        p ^= 1;
        return accA + accB;
    };
    (void)mid_g;      // (K7f only)
    // transposed DE layer (image in LDS) + the weight gradient of that layer from the very tiles the all-gather published:
    // acc[c] += delta(block (w+c) % NWV)^T (x) hT, hT = this wave's own input activations in operand layout
    constexpr bool DEFER = PREFETCH_ALL && Tune::TREAD_AHEAD && Tune::DEFER_DW && !ROLES;
    f4 pendT[DEFER ? NWV : 1], pend_h = f4{0.f, 0.f, 0.f, 0.f};
    constexpr bool PAIR = Tune::DW_PAIR && NWV >= 8 && (Tune::PAIR_REC || !REC);      // the paired dW arm of midT
    constexpr bool DEFER8 = PAIR && Tune::DEFER8;
    int pend_par = 0;
    auto dw_groups = [&](const int par, const f4 hT, f4 (&acc)[NWV]) {
        constexpr int DG = Tune::DW_PAIR <= 1 ? 2 : Tune::DW_PAIR;      // chunks per group
#pragma unroll
        for (int c = 0; c < NWV; c += DG) {
            f4 dTg[DG];
#pragma unroll
            for (int q = 0; q < DG; ++q) dTg[q] = get_row(tile(par, (w + c + q) & (NWV - 1)), roff);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int q = 0; q < DG; ++q) acc[c + q] = fm4(dTg[q][kk], hT[kk], acc[c + q]);
            if constexpr (BOUND) __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto flush = [&](f4 (&pacc)[NWV]) {
        if constexpr (DEFER8) dw_groups(pend_par, pend_h, pacc);
        if constexpr (DEFER) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int c = 0; c < NWV; ++c) pacc[c] = fm4(pendT[c][kk], pend_h[kk], pacc[c]);
        }
    };
    auto midT = [&](const int layer, const f4 d, const f4 hT, f4 (&acc)[NWV], f4 (*pacc)[NWV] = nullptr) -> f4 {
        put(tile(p, w), d);
        const f4* wl = wT + ((size_t)layer * NWV * NWV + w) * 64 + l;
        f4 wq = wl[0];
        constexpr bool WAH = ROLES && Tune::W_AHEAD;
        f4 wah[WAH ? NWV : 1];
        if constexpr (WAH) {
#pragma unroll
            for (int c = 1; c < NWV; ++c) wah[c] = wl[c * NWV * 64];
        }
        f4 accA = fm4(wq[0], d[0], f4{0.f, 0.f, 0.f, 0.f}), accB = fm4(wq[1], d[1], f4{0.f, 0.f, 0.f, 0.f});
        accA = fm4(wq[2], d[2], accA); accB = fm4(wq[3], d[3], accB);
        if constexpr (DEFER || DEFER8) { if (pacc) flush(*pacc); }
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
        if constexpr (PREFETCH_ALL && Tune::TREAD_AHEAD) {
            f4 vq[NWV], wqq[NWV], dTq[ROLES ? 1 : NWV];
#pragma unroll
            for (int c = 1; c < NWV; ++c) { vq[c] = getl(tile(p, (w + c) & (NWV - 1))); wqq[c] = WAH ? wah[WAH ? c : 0] : wl[c * NWV * 64]; }
            if constexpr (!ROLES) {
#pragma unroll
                for (int c = 0; c < NWV; ++c) dTq[c] = get_row(tile(p, (w + c) & (NWV - 1)), roff);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 1; c < NWV; ++c) {
                accA = fm4(wqq[c][0], vq[c][0], accA); accB = fm4(wqq[c][1], vq[c][1], accB);
                accA = fm4(wqq[c][2], vq[c][2], accA); accB = fm4(wqq[c][3], vq[c][3], accB);
            }
            if constexpr (ROLES) {
                (void)dTq; (void)hT; (void)acc;       // the gradient waves' work
            } else if constexpr (DEFER) {
#pragma unroll
                for (int c = 0; c < NWV; ++c) pendT[c] = dTq[c];
                pend_h = hT;
            } else {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int c = 0; c < NWV; ++c) acc[c] = fm4(dTq[c][kk], hT[kk], acc[c]);      // NWV independent chains
            }
            p ^= 1;
            return accA + accB;
        }
        if constexpr (Tune::DP_GROUP > 0 && NWV >= 8) {
            constexpr int PG = Tune::DP_GROUP > 0 ? Tune::DP_GROUP : 1;
#pragma unroll
            for (int c0 = 1; c0 < NWV; c0 += PG) {
                f4 vg[PG], wg[PG];
#pragma unroll
                for (int q = 0; q < PG; ++q) if (c0 + q < NWV) { vg[q] = getl(tile(p, (w + c0 + q) & (NWV - 1))); wg[q] = wl[(c0 + q) * NWV * 64]; }
#pragma unroll
                for (int q = 0; q < PG; ++q) if (c0 + q < NWV) {
                    accA = fm4(wg[q][0], vg[q][0], accA); accB = fm4(wg[q][1], vg[q][1], accB);
                    accA = fm4(wg[q][2], vg[q][2], accA); accB = fm4(wg[q][3], vg[q][3], accB);
                }
                if constexpr (BOUND) __builtin_amdgcn_sched_barrier(0);
            }
        } else
#pragma unroll
        for (int c = 1; c < NWV; ++c) {
            const f4 v = getl(tile(p, (w + c) & (NWV - 1)));
            wq = wl[c * NWV * 64];
            accA = fm4(wq[0], v[0], accA); accB = fm4(wq[1], v[1], accB);
            accA = fm4(wq[2], v[2], accA); accB = fm4(wq[3], v[3], accB);
            if constexpr (BOUND) { if (c % EVERY == EVERY - 1) __builtin_amdgcn_sched_barrier(0); }
        }
        if constexpr (PAIR) {
            if constexpr (DEFER8) { pend_par = p; pend_h = hT; }      // (the tiles of this parity stay intact until the exchange after next)
            else dw_groups(p, hT, acc);
        } else {
#pragma unroll
        for (int c = 0; c < NWV; ++c) {
            const f4 dT = get_row(tile(p, (w + c) & (NWV - 1)), roff);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[c] = fm4(dT[kk], hT[kk], acc[c]);
            if constexpr (BOUND) { if (c % EVERY == EVERY - 1) __builtin_amdgcn_sched_barrier(0); }
        }
        }
        p ^= 1;
        return accA + accB;
    };
    // split-K over the waves' own units (4 MFMAs)
    auto own4 = [&](const float (&wq)[4], const f4 h) -> f4 {
        f4 accA = fm4(wq[0], h[0], f4{0.f, 0.f, 0.f, 0.f}), accB = fm4(wq[1], h[1], f4{0.f, 0.f, 0.f, 0.f});
        accA = fm4(wq[2], h[2], accA); accB = fm4(wq[3], h[3], accB);
        return accA + accB;
    };
    // all-reduce of the output rows over the waves (fixed order): 2 rows (x-layout) or 4 rows (slot layout)
    auto allreduce2 = [&](const f2 part, const f2 init, f4 (*pacc)[NWV] = nullptr) -> f2 {
        f2* xb2 = reinterpret_cast<f2*>(tile(p, 0));
        xb2[w * 64 + l] = part;
        if constexpr (DEFER || DEFER8) { if (pacc) flush(*pacc); }
        lds_barrier();
        f2 out = init;
#pragma unroll
        for (int c = 0; c < NWV; ++c) out += xb2[c * 64 + l];
        p ^= 1;
        return out;
    };
    auto allreduce4 = [&](const f4 part, const f4 init, f4 (*pacc)[NWV] = nullptr) -> f4 {
        put(tile(p, w), part);
        if constexpr (DEFER || DEFER8) { if (pacc) flush(*pacc); }
        lds_barrier();
        f4 out = init;
#pragma unroll
        for (int c = 0; c < NWV; ++c) out += getl(tile(p, c));
        p ^= 1;
        return out;
    };
