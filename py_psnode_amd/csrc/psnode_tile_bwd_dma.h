// The LDS-DMA of a weight image of K4f / K7f, as text (see psnode_tile_bwd_chain.h): included in the kernel body in front of the first
// transfer.  In scope: NWV, wT, l, w.  Defines dma_layer and dma_wait.
    // LDS-DMA of one layer's image (0: W2, 1: W3) into its region: slot (layer, c, w) <- 64 lanes x 16 B, lane-linear.  The statement
    // first drains this wave's LDS reads (they are the only readers of these slots) and is invisible to the compiler's wait counts:
    // dma_wait() before the first use.
    const unsigned wT_lds = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(wT));
    const unsigned lane16 = 16u * (unsigned)l;
    auto dma_layer = [&](const f4* __restrict__ img, const int layer) {
#pragma unroll
        for (int c = 0; c < NWV; ++c) {
            const int slot = (layer * NWV + c) * NWV + w;
            // source = <uniform slot base in SGPRs> + <lane * 16 bytes>: one VGPR for all 32 slots (a per-lane 64-bit pointer per slot is
            // loop-invariant, and the compiler kept -- and spilled -- all of them)
            const uintptr_t sb = reinterpret_cast<uintptr_t>(img + (size_t)slot * 64);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)sb), hi = __builtin_amdgcn_readfirstlane((unsigned)(sb >> 32));
            const unsigned long long base = ((unsigned long long)hi << 32) | lo;
            const unsigned dst = __builtin_amdgcn_readfirstlane(wT_lds + (unsigned)slot * 1024u);
            unsigned keep;
            asm volatile(PSNODE_LDS_DMA_ASM
                         : "=&s"(keep) : "v"(lane16), "s"(dst), "s"(base) : "memory");
        }
    };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
