// Vertical sweep: the last stage of the fused schedule in MODE_SGBM_3WAY (mode 2: the paths W, E and N).  Included by sgbm.hip
// behind sgbm_diag.inc (uses its DiagJob, its buffer loads and its LDS helpers).
//
// With N as the only top-down path a column needs nothing of its neighbours: L_N(x, y) follows from L_N(x, y - 1) and C(x, y)
// alone.  The pass is therefore a plain grid of independent columns -- no strips, no hand-off, no control block, no boundary
// granules, no wait: nothing in here can give up, and the kernel never touches a control word (the pair's control block stays
// as k_sgbm_planes cleared it, so the post kernel behind reports a healthy sweep).
//
// Mapping, as k_sgbm_paths walks an N line: a column = one 16-lane DPP row (each lane NP packed registers = 2 NP disparities),
// four adjacent columns per wave, so a wave reads 4 * Dp * 2 contiguous bytes of C and as many of the W + E volume per image row.
// S = sat(L_W + L_E) + L_N goes through the diagonal sweep's winner logic unchanged (wta_count; the record of a pixel is written
// one row late, when the winner's two neighbour costs have come back from the two LDS rows of S the column keeps), and leaves the
// same two-word records: aux0 = minS << 8 | best, or -1 (uniqueness test failed, or every sum saturated), aux1 = S[best - 1] << 16
// | S[best + 1].  k_sgbm_post_rows / k_sgbm_fin read them as they read the diagonal sweep's.
//
// One wave per workgroup.  A pair has only ceil(W1 / 4) waves (288 at 1280 x 720, D = 128), each ONE dependent chain of H steps,
// and nothing is shared between waves: workgroups of one wave let the dispatcher spread them over as many CUs as there are, where a
// workgroup of four would put four chains on one CU and leave three CUs idle.  With one or two waves on a SIMD nothing hides a
// load but the wave's own prefetch: PF rows of BOTH streams are in flight (HBM-miss latency is ~900 cycles on an idle chip and more
// under load; a step is about 200 dependent packed / DPP / LDS instructions, measured 0.34 us per row at D = 128, so eight rows
// ahead up to 128 disparities is several latencies deep; the register file is no constraint at this occupancy, the depth drops
// with NP only to keep the unrolled body within the instruction cache).  Both streams are read for the last time here:
// non-temporal loads.  Lanes and rows that have nothing to load or store name an offset beyond the buffer descriptor's range (loads
// return 0, stores are dropped), so no lane-dependent branch guards a load or a store and the waits stay partial (the comment in
// k_sgbm_paths); the trip count is rounded up to whole groups of PF rows for the same reason.
//
// The job is a grid dimension (blockIdx.y) of a DiagJobs table, as the other stages of a sweep group take theirs: today every
// launch carries one job.
template <int NP, bool PAD>
__global__ void __launch_bounds__(64) k_sgbm_vert(DiagJobs jobs, SgbmGeom g)
{
    const DiagJob& job = jobs.j[blockIdx.y];
    extern __shared__ u32x4 s_vt[];                                     // [4 columns][2 rows][Dp] int16: S of this row and the previous
    const int lane = threadIdx.x & 63, q = lane >> 4, l16 = lane & 15;
    const int W1 = g.W1, H = g.H, Dp = g.Dp;
    const int x = (int)blockIdx.x * 4 + q;
    const bool col = x < W1;
    const int d0 = l16 * 2 * NP;
    unsigned padreg = 0;
    if constexpr (PAD) {
#pragma unroll
        for (int k = 0; k < NP; k++) padreg |= (unsigned)(d0 + 2 * k >= g.D) << k;
    }
    constexpr int RPS = NP * 2;                                         // registers per prefetched row
    constexpr int PF = RPS <= 8 ? 8 : RPS <= 12 ? 6 : 4;               // (16 at D = 128: 0.250 ms against 0.247: the chain sets the time)
    const uint32_t P1_2 = pk_rep(g.P1), P2_2 = pk_rep(g.P2);
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)job.C, 0, (int)job.vol_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rI = __builtin_amdgcn_make_buffer_rsrc((void*)job.in1, 0, (int)job.vol_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rA0 = __builtin_amdgcn_make_buffer_rsrc((void*)job.aux0, 0, (int)job.rec_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rA1 = __builtin_amdgcn_make_buffer_rsrc((void*)job.aux1, 0, (int)job.rec_bytes, 0x00020000);
    // byte offset of this lane's cells at row y (32 bits: the host refuses a volume of 4 GiB and more), one row down = rstride
    const uint32_t rstride = (uint32_t)W1 * (uint32_t)Dp * 2u;
    const uint32_t off0 = (uint32_t)(x * Dp + d0) * 2u;
    LV<NP> cbuf[PF], ibuf[PF];
#pragma unroll
    for (int k = 0; k < PF; k++) {
        const uint32_t o = (col && k < H) ? off0 + (uint32_t)k * rstride : DG_OOB;
        cbuf[k] = lv_bload_nt<NP>(rC, o);
        ibuf[k] = lv_bload_nt<NP>(rI, o);
        // The way into the loop issues what a step of the loop issues, in the loop's order: two loads, then two (dropped) record
        // stores, pinned by a scheduling fence.  The compiler counts the loop's first waits against the shorter of the two ways
        // in; left to itself it loads row 0 LAST here, and every group of PF rows then begins by draining the whole queue
        // (s_waitcnt vmcnt(0): seen in the code generated for this kernel, gone with these lines).
        __builtin_amdgcn_raw_buffer_store_b32(0, rA0, DG_OOB, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(0, rA1, DG_OOB, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t poff = off0 + (uint32_t)PF * rstride;                      // row PF, unchecked
    lds_u8* const myS = (lds_u8*)s_vt + (size_t)q * 2 * Dp * 2;         // two rows of S of this column

    LV<NP> Lp;                                                          // the predecessor above the image: zeros, pads MAX_COST
#pragma unroll
    for (int k = 0; k < NP; k++) Lp.r[k] = ((padreg >> k) & 1u) ? MAXC2 : 0u;
    uint32_t delta2 = P2_2;
    // the winner of the previous row's pixel (see dg_strip: the same record, the same one-row delay)
    int spar = 0, pkey = 0, pcnt = 0, pT = 0;
    bool plive = false;
    uint32_t paoff = 0;
    uint32_t aoff = (uint32_t)(x + g.minX1) * 4u;                       // byte offset of the record of this column's pixel at row 0
    const uint32_t astride = (uint32_t)g.W * 4u;
    auto finish_record = [&]() {
        const int pbest = pkey & 255, pminS = pkey >> 8;
        const int i0 = max(pbest - 1, 0), i1 = min(pbest + 1, Dp - 1);
        const lds_u8* const prevS = myS + (size_t)(spar ^ 1) * Dp * 2;
        const int sm = (int)*(const lds_u16*)(prevS + i0 * 2), sp = (int)*(const lds_u16*)(prevS + i1 * 2);
        // costs below T among the excluded ones: the winner itself and its neighbours where they exist
        const int excl = (int)(pminS < pT) + (int)(pbest > 0 && sm < pT) + (int)(pbest < g.D - 1 && sp < pT);
        const uint32_t so = (plive && l16 == 0) ? paoff : DG_OOB;      // (lanes without a record to write: out of range, dropped)
        // (every sum saturated at 32767: no winner, whatever the uniqueness ratio)
        __builtin_amdgcn_raw_buffer_store_b32((pcnt > excl || pminS >= MAXC) ? -1 : pkey, rA0, so, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32((int)(((uint32_t)sm << 16) | (uint32_t)sp), rA1, so, 0, 0);
    };
    // straight-line body: no branch between a prefetch and its use (dg_strip says why); the surplus rows of the last group are dead
    // (their loads return zeros, their records go nowhere)
    const int yend = (H + PF - 1) / PF * PF;
    for (int y0 = 0; y0 < yend; y0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int y = y0 + k;
            const bool live = col && y < H;
            LV<NP> S = ibuf[k];
            const LV<NP> Cv = cbuf[k];
            const LV<NP> L = path_step2<NP, PAD>(Cv, Lp, delta2, P1_2, padreg);
            delta2 = pk_rep_add(row_min_u32(lane_min16<NP>(L)), P2_2);
            Lp = L;
#pragma unroll
            for (int i = 0; i < NP; i++) S.r[i] = pk_add_sat(S.r[i], L.r[i]);
            // the row PF steps ahead goes into the registers this step has just finished with (behind a scheduling fence: dg_strip)
            __builtin_amdgcn_sched_barrier(0);
            {
                const uint32_t o = (col && y + PF < H) ? poff : DG_OOB;
                cbuf[k] = lv_bload_nt<NP>(rC, o);
                ibuf[k] = lv_bload_nt<NP>(rI, o);
                poff += rstride;
            }
            finish_record();                                            // the previous row's pixel
            int minS, best, cnt, T;
            wta_count<NP, PAD>(S, g, lane, minS, best, cnt, T);
            dg_lds_store<NP>(myS + (size_t)spar * Dp * 2 + d0 * 2, S);
            pkey = (minS << 8) | best;
            pcnt = cnt;
            pT = T;
            plive = live;
            paoff = aoff;
            aoff += astride;
            spar ^= 1;
        }
    }
    finish_record();                                                    // the last row's pixel (dead when the trip count was rounded up)
}
