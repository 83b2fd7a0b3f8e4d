// The census cost of the SGBM front (vo_set_sgbm_cost: VO_SGBM_COST_CENSUS), included by sgbm.hip behind the BT front's kernels.
// Two kernels stand in the place of k_sgbm_planes + k_sgbm_cost_sweep / k_sgbm_cost_generic; everything behind them reads C alone.
//   k_census       one 64-bit signature per pixel and image: bit b = (neighbour b of the cw x ch window < centre), rows and columns
//                  replicated at the border.  The left image's signatures lie where planesL lies (8 bytes per pixel), the right
//                  image's in the first third of planesR: nothing is allocated for this cost.  The kernel also does everything
//                  k_sgbm_planes does on the side (the P2 row behind C, the sweep's control block, keepL / keepR, d2key).
//   k_census_cost  Hamming pixel cost + (2*SW2+1)^2 box sum + P2, C written once.  The organisation is k_sgbm_cost_sweep's: one lane =
//                  one disparity PAIR in packed int16x2, a wave walks XT columns down a band of rows, the horizontal window slides
//                  in registers, the vertical one through a ring (registers up to 5 x 5, LDS beyond).  The right image's
//                  signatures of the row segment the wave needs -- NC + 127 positions, clamped to the row -- are staged in LDS
//                  once per row, split by parity: lane l reads positions x - minD - 2l and one less, so each read takes consecutive
//                  8-byte words for consecutive lanes.  Every strip takes this one path: border strips clamp where they load.
// The largest block cost is 121 * 62 = 7502, + P2 <= 8000: no packed half can overflow.

#define CEN_TX 64
#define CEN_TY 16
#define CEN_HX 4          // halo of the largest window (9 x 7); smaller windows read less of it
#define CEN_HY 3

__global__ void __launch_bounds__(256) k_census(FrontJobs jobs, int W, int H, int rw, int rh, int sw_ctl_words, int dummy_words, uint32_t P2_2)
{
    const FrontJob& J = jobs.j[blockIdx.z];
    const uint8_t* __restrict__ const L = J.L;
    const uint8_t* __restrict__ const R = J.R;
    uint64_t* __restrict__ const SL = (uint64_t*)J.planesL;
    uint64_t* __restrict__ const SR = (uint64_t*)J.planesR;
    __shared__ uint8_t tile[2][CEN_TY + 2 * CEN_HY][CEN_TX + 2 * CEN_HX];
    const int tid = threadIdx.x;
    // what k_sgbm_planes leaves behind for the kernels after the front: the row of P2 cells (= cost 0) behind the used part of C,
    // and a zeroed control block for this run's sweeps
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int i = tid; i < dummy_words; i += blockDim.x) J.dummy[i] = P2_2;
        for (int i = tid; i < sw_ctl_words; i += blockDim.x) J.sw_ctl[i] = 0;
    }
    const int x0 = blockIdx.x * CEN_TX, y0 = blockIdx.y * CEN_TY;
    constexpr int TW = CEN_TX + 2 * CEN_HX, TH = CEN_TY + 2 * CEN_HY;
    for (int i = tid; i < TW * TH; i += blockDim.x) {
        const int ty = i / TW, tx = i - ty * TW;
        const int gx = min(max(x0 + tx - CEN_HX, 0), W - 1), gy = min(max(y0 + ty - CEN_HY, 0), H - 1);
        const size_t gi = (size_t)gy * W + gx;
        tile[0][ty][tx] = L[gi];
        tile[1][ty][tx] = R[gi];
    }
    __syncthreads();
    const int tx = tid & 63, x = x0 + tx;
    if (x >= W) return;
    for (int ty = tid >> 6; ty < CEN_TY; ty += 4) {
        const int y = y0 + ty;
        if (y >= H) break;
        const size_t i = (size_t)y * W + x;
        const int cl = tile[0][ty + CEN_HY][tx + CEN_HX], cr = tile[1][ty + CEN_HY][tx + CEN_HX];
        uint64_t sl = 0, sr = 0;
        int bit = 0;
        for (int dy = -rh; dy <= rh; dy++)
            for (int dx = -rw; dx <= rw; dx++) {
                if (dx == 0 && dy == 0) continue;
                sl |= (uint64_t)(tile[0][ty + CEN_HY + dy][tx + CEN_HX + dx] < cl) << bit;
                sr |= (uint64_t)(tile[1][ty + CEN_HY + dy][tx + CEN_HX + dx] < cr) << bit;
                bit++;
            }
        SL[i] = sl;
        SR[i] = sr;
        // (a pair read where it lies: its copy into the frame slot; the unfused schedule's disp2 candidates start empty)
        if (J.keepL) { J.keepL[i] = (uint8_t)cl; J.keepR[i] = (uint8_t)cr; }
        if (J.d2key) J.d2key[i] = D2_EMPTY;
    }
}

template <int XT, int SW2>
__global__ void __launch_bounds__(128) k_census_cost(FrontJobs jobs, SgbmGeom g, int TY)
{
    const FrontJob& J = jobs.j[blockIdx.y];
    const uint64_t* __restrict__ const SL = (const uint64_t*)J.planesL;
    const uint64_t* __restrict__ const SR = (const uint64_t*)J.planesR;
    int16_t* __restrict__ const C = J.C;
    constexpr int WIN = 2 * SW2 + 1, NC = XT + 2 * SW2;
    constexpr int NSEG = NC + 127, NJ = (NSEG + 1) / 2;       // staged positions of a row; words per parity
    constexpr bool RING_REGS = WIN <= 5;
    extern __shared__ uint64_t s_cen[];   // [waves][WIN][XT][64] u32 when the ring lives here, then the staging [waves][2][NJ] u64
    uint32_t ringv[RING_REGS ? WIN : 1][XT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    uint32_t* const ring = (uint32_t*)s_cen + (size_t)wv * WIN * XT * 64 + lane;              // (LDS variant only)
    uint64_t* const stage = s_cen + (RING_REGS ? 0 : (size_t)nwv * WIN * XT * 32) + (size_t)wv * 2 * NJ;
    const int dpl = threadIdx.x;                  // disparity pair index (padded layout)
    const bool pad = 2 * dpl >= g.D;
    // XCD-aware tile order, as in k_sgbm_cost_sweep
    const int gx = (g.W1 + XT - 1) / XT, total = gx * ((g.H + TY - 1) / TY);
    const int chunk = (total + 7) >> 3, tile = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (tile >= total) return;
    const int tbx = tile % gx, tby = tile / gx;
    const int xa = tbx * XT, ya = tby * TY;
    const int yend = min(ya + TY, g.H);
    const int nrows = (yend - ya) + 2 * SW2;
    // image column of halo column k: the band clamps it (the box sum replicates the band's border columns)
    auto ximg_of = [&](int k) { return min(max(xa - SW2 + k, 0), g.W1 - 1) + g.minX1; };
    const int xlo = ximg_of(0);
    const int pbase = xlo - g.minD - 128 * wv - 127;          // right-image position of staged entry 0: lane 63's second cell at halo column 0
    const int xrun = ximg_of(min(lane, NC - 1));              // lane k < NC fetches the left signature of halo column k
    int pos[3];
#pragma unroll
    for (int q = 0; q < 3; q++) pos[q] = min(max(pbase + lane + 64 * q, 0), g.W - 1);
    const bool third = lane + 128 < NSEG;
    uint64_t* const st_wr = stage + (lane & 1) * NJ + (lane >> 1);     // entry i lies at [(i & 1) * NJ + (i >> 1)]; i = lane + 64 q
    auto row_of = [&](int rr) { return (size_t)min(max(ya - SW2 + rr, 0), g.H - 1) * g.W; };
    uint64_t nxt[3], nl;
    auto fetch = [&](int rr) {
        const size_t rowi = row_of(rr);
        nxt[0] = SR[rowi + pos[0]];
        nxt[1] = SR[rowi + pos[1]];
        nxt[2] = third ? SR[rowi + pos[2]] : 0;
        nl = SL[rowi + xrun];
    };

    uint32_t acc[XT];
#pragma unroll
    for (int j = 0; j < XT; j++) acc[j] = pk_rep(g.P2);

    fetch(0);
    for (int rr0 = 0; rr0 < nrows; rr0 += WIN) {
#pragma unroll RING_REGS ? WIN : 1
    for (int slot = 0; slot < WIN; slot++) {
        const int rr = rr0 + slot;
        if (rr >= nrows) break;                                        // (uniform)
        __builtin_amdgcn_wave_barrier();                               // (the previous row's reads lie before these writes)
        st_wr[0] = nxt[0];
        st_wr[32] = nxt[1];
        if (third) st_wr[64] = nxt[2];
        const uint32_t ll = (uint32_t)nl, lh = (uint32_t)(nl >> 32);
        __builtin_amdgcn_wave_barrier();
        fetch(min(rr + 1, nrows - 1));
        uint32_t pc[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            // this lane's two cells at halo column k: d = 2 dpl at entry t - 2 lane, d + 1 at the entry below it
            const int t = ximg_of(k) - xlo + 127;                      // (uniform)
            const int jj = (t >> 1) - lane;
            const uint64_t r0 = (t & 1) ? stage[NJ + jj] : stage[jj];
            const uint64_t r1 = (t & 1) ? stage[jj] : stage[NJ + jj - 1];
            const uint64_t sl = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)ll, k) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)lh, k) << 32);
            pc[k] = (uint32_t)__builtin_popcountll(sl ^ r0) | ((uint32_t)__builtin_popcountll(sl ^ r1) << 16);
        }
        // horizontal sliding sums -> vertical ring / accumulators
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < WIN; k++) s = pk_add(s, pc[k]);
#pragma unroll
        for (int j = 0; j < XT; j++) {
            if (j > 0) s = pk_sub(pk_add(s, pc[j + WIN - 1]), pc[j - 1]);
            if constexpr (RING_REGS) {
                if (rr >= WIN) acc[j] = pk_sub(acc[j], ringv[slot][j]);   // the row leaving the window
                acc[j] = pk_add(acc[j], s);
                ringv[slot][j] = s;
            } else {
                uint32_t* cell = ring + (size_t)(slot * XT + j) * 64;
                if (rr >= WIN) acc[j] = pk_sub(acc[j], *cell);
                acc[j] = pk_add(acc[j], s);
                *cell = s;
            }
        }
        if (rr >= WIN - 1) {
            const int y = ya + rr - (WIN - 1);
#pragma unroll
            for (int j = 0; j < XT; j++) {
                const int x1 = xa + j;
                if (x1 < g.W1 && 2 * dpl < g.Dp)
                    *(uint32_t*)(C + ((size_t)y * g.W1 + x1) * g.Dp + 2 * dpl) = pad ? MAXC2 : acc[j];
            }
        }
    }
    }
}

// signatures and cost volume of n pairs of one geometry on the current stream: one launch each
static int census_front_launch(vo_ctx* ctx, const FrontJobs& jobs, int n, const SgbmGeom& g)
{
    const int w = g.W, h = g.H;
    hipLaunchKernelGGL(k_census, dim3(div_up(w, CEN_TX), div_up(h, CEN_TY), n), dim3(256), 0, ctx->stream, jobs, w, h, ctx->sg_cost.cw / 2,
                       ctx->sg_cost.ch / 2, ctx->sw_ctl_words, g.Dp / 2, pk_rep_host(g.P2));
    const int bx = ((g.Dp / 2 + 63) / 64) * 64;
    const int TY = ctx->tune_sweep_ty;
    const int nw = bx / 64;
#define LAUNCH_CENSUS(XT, SW)                                                                                                  \
    hipLaunchKernelGGL((k_census_cost<XT, SW>), dim3(8 * div_up(div_up(g.W1, XT) * div_up(h, TY), 8), n), dim3(bx),             \
                       (size_t)nw * (((2 * SW + 1) <= 5 ? 0 : (2 * SW + 1) * XT * 64) * 4 + ((XT + 2 * SW + 127 + 1) / 2) * 16), ctx->stream, jobs, g, TY)
    if (ctx->tune_diag_dbg & 4) {                // development only (VO_DIAG_DEBUG), as in front_launch
    } else
    switch (g.SW2) {
        case 0: LAUNCH_CENSUS(8, 0); break;
        case 1: LAUNCH_CENSUS(8, 1); break;
        case 2: LAUNCH_CENSUS(8, 2); break;
        case 3: LAUNCH_CENSUS(8, 3); break;
        case 4: LAUNCH_CENSUS(8, 4); break;
        case 5: LAUNCH_CENSUS(8, 5); break;
        default: return vo_fail(ctx, VO_E_ARG, "blockSize > 11 is not supported");      // (vo_set_sgbm refuses it already)
    }
#undef LAUNCH_CENSUS
    VO_CHECK_LAUNCH(ctx);
    return VO_OK;
}
