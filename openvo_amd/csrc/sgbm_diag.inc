// Diagonal sweep: the three top-down path directions -- NW (x-1,y-1), N (x,y-1), NE (x+1,y-1), or their mirror images
// SW, S, SE when REV -- computed TOGETHER in one pass over the cost volume and never stored: the pass adds the volume(s)
// aggregated beforehand (W + E as one volume from k_sgbm_we; MODE_HH: also the reverse pass's sum) and either runs the
// winner-take-all on the total (WTA) or stores the total (REV pass of MODE_HH, which the forward pass then adds).
// Included by sgbm.hip (uses its packed-int16 helpers).
//
// Why diagonal.  In image columns the three predecessors of (x, y) sit at x-1, x, x+1 of the row above: a column's
// state depends on BOTH neighbours, so column tiles need each other both ways every row.  In the skewed column
// uu = x - y + (H-1) the same predecessors sit at uu, uu+1, uu+2: NW stays in its own lane (registers), N and NE
// come from the right only.  The sweep is therefore a chain of strips of UW skewed columns in which strip j needs,
// per row, three records (L_N of one column, L_NE of two) from strip j+1's previous row and nothing from strip j-1.
//
// Mapping.  A strip = one workgroup of NWC compute waves + one helper wave.  Compute wave w owns the four skewed
// columns 4w..4w+3 (a column = one 16-lane DPP row, each lane NP packed registers = 2 NP disparities) and walks the
// strip's rows top to bottom; at row y its pixel is x = uu - (H-1) + y.  The waves of a strip are NOT barrier-locked (see
// DG_RING below): L_N / L_NE of the rows just computed lie in a ring of DG_RING row buffers in LDS, a row reads columns
// +1 / +2 of the previous one behind its right neighbour's progress word; columns UW, UW+1 of a buffer (the halo) are
// filled by the helper wave from the boundary buffer in HBM, which strip j+1's helper writes from ITS columns 0 and 1.
// A pixel outside the image
// carries the border state (zeros, pads MAX_COST: stereosgbm.cpp's zero-initialised Lr borders), so "predecessor
// outside" needs no special case anywhere.
//
// Hand-off between strips (MI355X_MICROARCH.md, inter-workgroup visibility, data-tagged granules): a record travels as
// naturally aligned 8-byte granules {data dword, tag dword}, each written by one agent-scope (sc1) store and read by an
// agent-scope load of the helper wave only; the tag is this launch's sequence number of the workspace, so a granule is
// valid exactly when its tag matches: no flag, no counter, no wait on the producing side.  The importing helper issues
// its loads DG_AHEAD rows ahead and re-polls only the rows that had not arrived; a strip thus trails its right
// neighbour by a few rows.  Every wait is bounded: after `spin_limit` polls (2^22) a wave raises word 1 of ITS PAIR's control
// block (DiagJob::ctl) and stops waiting, the pair's other waves see the word and stop waiting too: every workgroup terminates,
// the results of THIS pair are undefined.  k_sgbm_fin then marks the slot the pair fills (FrameSlot::sweep_word): whoever picks
// up anything computed from that disparity gets VO_E_SWEEP instead.  The word is per pair and per run (k_sgbm_planes of the
// workspace's next run clears it; a strip only ever waits for strips of its own pair, so the other pairs of a launch lose
// nothing): the next pair is exact again.
//
// Scheduling.  Workgroups are persistent: each takes (pair, strip) work items off a ticket counter, right-most strip
// first, so a strip only ever waits for a strip that a running (or finished) workgroup has already taken -- no wait
// depends on dispatch order or residency.  One launch can carry several queued pairs (DiagJobs; the look-ahead path's sweep
// groups, sgbm.hip): occupancy then no longer depends on the number of streams.  Tickets run through the pairs first -- ticket
// t is strip t / n from the right of pair t % n -- so the pairs advance side by side and the launch takes about as long as one
// pair's.  The ticket counter and the strip timeline (pair 0's) live in the control block the launch is given.
//
// HBM traffic of the pass in units of one volume: C read once, the input volume read once, + 6 / UW for the boundary
// granules (3 records of 2 x 2 bytes per cell, written and read) -- against one read of C per direction and a write +
// a read of every L in the line scheme.
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) volatile int lds_vint;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;

#ifndef DG_AHEAD
#define DG_AHEAD 4                 // boundary rows the importing helper keeps in flight
#endif
#define DG_MAXJOBS 12

struct DiagJob {
    const int16_t* C;      // cost volume (+P2)
    const int16_t* in1;    // the volume aggregated beforehand (W + E; MODE_HH forward pass: the reverse pass's output)
    int16_t* sout;         // !WTA: in1 + the three directions of this pass goes here
    uint64_t* bnd;         // boundary granules [strip][H + 1 rows][NP][64 lanes]
    int* aux0;             // WTA records (k_sgbm_fin)
    int* aux1;
    uint32_t tag;          // this launch's sequence number in the workspace (never 0)
    int sink;              // index of 64 spare words behind aux0 / aux1 (stores of lanes that have no record to write)
    int dbg;               // development only (VO_DIAG_DEBUG): bit 0 = import nothing, bit 1 = export nothing (results are then wrong)
    int spin_limit;        // polls before a wait is declared dead (vo_ctx::tune_spin_limit)
    uint32_t vol_bytes;    // bytes of one volume + one more pixel's cells (behind C: the dummy row holding P2, k_sgbm_planes)
    uint32_t rec_bytes;    // bytes of one record array (64 spare words included)
    int* ctl;              // this pair's own control block: word 1 = its sticky give-up flag (the pair's post kernel reads it)
};

// buffer addressing for the sweep's streams: a descriptor (scalar registers) + one 32-bit byte offset per lane -- no 64-bit
// vector address arithmetic in the row loop, and a lane with nothing to load or store simply names an offset beyond the
// descriptor's range (loads return 0, stores are dropped): no dump area, no selects on loaded values
#define DG_OOB 0xFFFFFF00u
template <int NP>
__device__ __forceinline__ LV<NP> lv_bload_nt(__amdgpu_buffer_rsrc_t r, uint32_t boff)
{
    LV<NP> v;
    if constexpr (NP % 4 == 0) {
#pragma unroll
        for (int k = 0; k < NP / 4; k++) {
            const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r, boff + 16 * k, 0, 2);
            v.r[4 * k] = t.x; v.r[4 * k + 1] = t.y; v.r[4 * k + 2] = t.z; v.r[4 * k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; k++) v.r[k] = __builtin_amdgcn_raw_buffer_load_b32(r, boff + 4 * k, 0, 2);
    }
    return v;
}
template <int NP>
__device__ __forceinline__ void lv_bstore_nt(__amdgpu_buffer_rsrc_t r, uint32_t boff, const LV<NP>& v)
{
    if constexpr (NP % 4 == 0) {
#pragma unroll
        for (int k = 0; k < NP / 4; k++) {
            const u32x4 t = { v.r[4 * k], v.r[4 * k + 1], v.r[4 * k + 2], v.r[4 * k + 3] };
            __builtin_amdgcn_raw_buffer_store_b128(t, r, boff + 16 * k, 0, 2);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; k++) __builtin_amdgcn_raw_buffer_store_b32(v.r[k], r, boff + 4 * k, 0, 2);
    }
}
struct DiagJobs {
    int n, nstrips;
    DiagJob j[DG_MAXJOBS];
};

template <int NP>
__device__ __forceinline__ LV<NP> dg_lds_load(const lds_u8* p)
{
    LV<NP> v;
    if constexpr (NP % 4 == 0) {
#pragma unroll
        for (int c = 0; c < NP / 4; c++) {
            const u32x4 t = *(const lds_u32x4*)(p + c * 16);
            v.r[4 * c] = t.x; v.r[4 * c + 1] = t.y; v.r[4 * c + 2] = t.z; v.r[4 * c + 3] = t.w;
        }
    } else if constexpr (NP % 2 == 0) {
#pragma unroll
        for (int c = 0; c < NP / 2; c++) {
            const u32x2 t = *(const lds_u32x2*)(p + c * 8);
            v.r[2 * c] = t.x; v.r[2 * c + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < NP; r++) v.r[r] = *(const lds_u32*)(p + r * 4);
    }
    return v;
}
template <int NP>
__device__ __forceinline__ void dg_lds_store(lds_u8* p, const LV<NP>& v)
{
    if constexpr (NP % 4 == 0) {
#pragma unroll
        for (int c = 0; c < NP / 4; c++) {
            const u32x4 t = { v.r[4 * c], v.r[4 * c + 1], v.r[4 * c + 2], v.r[4 * c + 3] };
            *(lds_u32x4*)(p + c * 16) = t;
        }
    } else if constexpr (NP % 2 == 0) {
#pragma unroll
        for (int c = 0; c < NP / 2; c++) {
            const u32x2 t = { v.r[2 * c], v.r[2 * c + 1] };
            *(lds_u32x2*)(p + c * 8) = t;
        }
    } else {
#pragma unroll
        for (int r = 0; r < NP; r++) *(lds_u32*)(p + r * 4) = v.r[r];
    }
}

// the strip's one barrier per work item (after the LDS state has been initialised)
__device__ __forceinline__ void dg_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#define DG_RING 4                  // rows of L_N / L_NE a strip keeps in LDS (power of two)
#define DG_GLANES 48               // granules per register of one (strip, row) hand-off block: three records x 16 lanes
#define DG_BIG (1 << 29)
// LDS control words of a strip: [0] work item, [1] abort, [2] rows imported (halo rows r < value are in the ring), [3] rows
// exported, [4 + w] rows published by compute wave w, [4 + NWC + w] "gave up waiting" (sticky) of wave w
//
// The waves of a strip are NOT barrier-locked: every wave walks its rows at its own pace and waits -- rarely -- on the progress
// word of its right neighbour (whose previous row it reads) and of its left neighbour (who must be done with the ring slot it is
// about to overwrite).  The slow path of such a wait is ONE opaque asm statement: a compiler-visible spin loop between the
// prefetch loads and their uses would make hipcc drain the whole vector-memory queue at the join, every row.  Spins until
// *lds_addr >= need; after DG_SPIN_LIMIT polls it sets the wave's `dead` word and from then on the wave never waits again
// (results undefined, error word raised at the end, no hang).
__device__ __forceinline__ int dg_spin(uint32_t lds_addr, int need, uint32_t dead_addr, int spin_limit)
{
    // (both addresses are wave-uniform: they travel in scalar registers, the loop borrows two vector registers)
    int spins, cur;
    uint32_t tmp, one;
    asm volatile("s_mov_b32 %0, 0\n"
                 "1:\n\t"
                 "v_mov_b32 %2, %4\n\t"
                 "ds_read_b32 %2, %2\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "s_nop 0\n\t"
                 "v_readfirstlane_b32 %1, %2\n\t"
                 "s_cmp_ge_i32 %1, %6\n\t"
                 "s_cbranch_scc1 3f\n\t"
                 "v_mov_b32 %2, %5\n\t"
                 "ds_read_b32 %2, %2\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "s_nop 0\n\t"
                 "v_readfirstlane_b32 %1, %2\n\t"
                 "s_cmp_lg_u32 %1, 0\n\t"
                 "s_cbranch_scc1 3f\n\t"
                 "s_add_i32 %0, %0, 1\n\t"
                 "s_cmp_lt_i32 %0, %7\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "v_mov_b32 %2, %5\n\t"
                 "v_mov_b32 %3, 1\n\t"
                 "ds_write_b32 %2, %3\n\t"
                 "s_branch 3f\n"
                 "2:\n\t"
                 "s_sleep 1\n\t"
                 "s_branch 1b\n"
                 "3:\n"
                 : "=&s"(spins), "=&s"(cur), "=&v"(tmp), "=&v"(one)
                 : "s"(__builtin_amdgcn_readfirstlane((int)lds_addr)), "s"(__builtin_amdgcn_readfirstlane((int)dead_addr)),
                   "s"(__builtin_amdgcn_readfirstlane(need)), "s"(__builtin_amdgcn_readfirstlane(spin_limit))
                 : "scc", "memory");
    return spins;
}

template <int N, typename F>
__device__ __forceinline__ void dg_static_for(F&& f)
{
    if constexpr (N > 0) {
        dg_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// rows [ys, ye) in which strip `strip` has at least one pixel inside the image
__device__ __forceinline__ void dg_rows(int strip, int UW, int W1, int H, int& ys, int& ye)
{
    const int uu0 = strip * UW;
    ys = max(0, (H - 1) - (uu0 + UW - 1));
    ye = min(H, W1 + (H - 1) - uu0);
}

// ---- the helper wave of a strip: exports the strip's left edge, imports the right neighbour's ---------------------------
template <int NP, int NWC>
__device__ __forceinline__ void dg_helper(const DiagJob& job, const SgbmGeom& g, int strip, int nstrips, int* __restrict__ ctl,
                                          lds_u8* bufs, lds_vint* W, unsigned padreg, int stats_words)
{
    constexpr int UW = 4 * NWC, CW = UW + 2;
    const int lane = threadIdx.x & 63, q = lane >> 4, l16 = lane & 15;
    const int W1 = g.W1, H = g.H, Dp = g.Dp;
    const int d0 = l16 * 2 * NP;
    const size_t bufsz = (size_t)2 * CW * Dp * 2;                       // bytes of one ring row (two directions)
    int ys, ye, nys = 0, nye = 0;
    dg_rows(strip, UW, W1, H, ys, ye);
    const bool has_nb = strip + 1 < nstrips;
    if (has_nb) dg_rows(strip + 1, UW, W1, H, nys, nye);
    // DPP row v of this wave moves record v: 0 = L_N of column 0 / halo column UW, 1 = L_NE of column 0 / UW,
    // 2 = L_NE of column 1 / UW + 1 (row 3 carries a copy of row 2's record in granules of its own)
    const int v = q < 3 ? q : 2;
    const int vdir = v == 0 ? 0 : 1, vcol = v == 2 ? 1 : 0;
    const size_t GR = (size_t)DG_GLANES * NP;                           // granules of one (strip, row) block: [NP][48 lanes], so that every
                                                                        // store / load instruction of this wave covers 512 contiguous bytes
    // a strip's block has H + 1 rows: row H is a dump row
    // (DPP row 3 moves a copy of row 2's record: its lanes name row 2's granules -- same addresses, same data, so the copy costs
    // no traffic: a block is 48 granules per register, 384 contiguous bytes per instruction)
    const int glane = q < 3 ? lane : lane - 16;
    const uint64_t* const src = job.bnd + (size_t)(has_nb ? strip + 1 : strip) * (H + 1) * GR + glane;
    uint64_t* const dst = job.bnd + (size_t)strip * (H + 1) * GR + glane;
    const uint32_t lds_exp = (uint32_t)(((size_t)vdir * CW + vcol) * Dp + d0) * 2;          // + ring slot * bufsz
    const uint32_t lds_imp = (uint32_t)(((size_t)vdir * CW + UW + vcol) * Dp + d0) * 2;
    LV<NP> border;
#pragma unroll
    for (int k = 0; k < NP; k++) border.r[k] = ((padreg >> k) & 1u) ? MAXC2 : 0u;
    const uint32_t tag = job.tag;
    const bool dbg_noimp = (job.dbg & 1) != 0, dbg_noexp = (job.dbg & 2) != 0;

    auto need = [&](int r) -> bool { return has_nb && r >= nys && r < nye && r + 1 < ye && !dbg_noimp; };
    auto fetch = [&](int r, uint64_t* gq) {        // (any row index: clamped into the block, the caller knows whether it counts)
        const uint64_t* p = src + (size_t)min(max(r, 0), H - 1) * GR;
#pragma unroll
        for (int k = 0; k < NP; k++) gq[k] = __hip_atomic_load(p + k * DG_GLANES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto arrived = [&](const uint64_t* gq) -> bool {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NP; k++) ok = ok && (uint32_t)(gq[k] >> 32) == tag;
        return __ballot(!ok) == 0ull;
    };
    int exp_next = ys;                             // next row of this strip to export
    int spins = 0, misses = 0;
    bool dead = false;
    auto give_up = [&]() -> bool {
        if (++spins > job.spin_limit ||
            ((spins & 255) == 0 && __builtin_amdgcn_readfirstlane(__hip_atomic_load(job.ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) {
            dead = true;                           // (or somebody else of this pair did): never wait again
            if (lane == 0) atomicExch(job.ctl + 1, 1);
            W[1] = 1;
        }
        return dead;
    };
    // every row compute wave 0 has published and that has not been sent yet: out of its ring slot, as tagged granules
    auto service_exports = [&]() {
        const int p0 = __builtin_amdgcn_readfirstlane(W[4]);
        bool any = false;
        while (exp_next < ye && exp_next < p0) {
            const LV<NP> L = dg_lds_load<NP>(bufs + (size_t)(exp_next & (DG_RING - 1)) * bufsz + lds_exp);
            uint64_t* p = dst + (size_t)(dbg_noexp ? H : exp_next) * GR;
#pragma unroll
            for (int k = 0; k < NP; k++)
                __hip_atomic_store(p + k * DG_GLANES, (uint64_t)L.r[k] | ((uint64_t)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            exp_next++;
            any = true;
        }
        if (any) {                                 // (the stores above consumed what the LDS reads returned: the slots are free again)
            asm volatile("" ::: "memory");
            if (lane == 0) W[3] = exp_next;
        }
    };

    uint64_t ring[DG_AHEAD][NP];
    const int r0 = ys - 1, rimp = ye - 1;          // rows r0 .. rimp - 1 of the neighbour feed this strip's rows ys .. ye - 1
    dg_static_for<DG_AHEAD>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        fetch(r0 + k, ring[k]);
    });
    // timeline of this strip for vo_sgbm_sweep_stats (100 MHz ticks): start, end, failed polls, ticks spent waiting for granules
    const uint32_t t_begin = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t t_wait = 0;
    for (int rb = r0; rb < rimp; rb += DG_AHEAD) {
        dg_static_for<DG_AHEAD>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const int r = rb + k;
            if (r < rimp) {                                             // (wave-uniform)
                const bool want = need(r);
                bool asked_again = false;
                uint32_t tw0 = 0;
                for (;;) {
                    service_exports();
                    // the halo of ring slot r is free once the last compute wave has finished row r - DG_RING + 1 (which read it)
                    const bool space = __builtin_amdgcn_readfirstlane(W[4 + NWC - 1]) >= r - DG_RING + 2;
                    const bool have = !want || dead || arrived(ring[k]);
                    if (space && have) break;
                    if (!have) {
                        // this row had not arrived when it was asked for, DG_AHEAD rows ago: the strip runs close behind its
                        // neighbour and the rows asked for since then were asked for too early as well -- ask for all of them
                        // again once, then keep polling this one
                        if (!asked_again) {
                            asked_again = true;
                            misses++;
                            tw0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
                            dg_static_for<DG_AHEAD>([&](auto ic) {
                                constexpr int i = decltype(ic)::value;
                                fetch(r + i, ring[(k + i) % DG_AHEAD]);
                            });
                        } else
                            fetch(r, ring[k]);
                    }
                    __builtin_amdgcn_s_sleep(1);
                    if (give_up()) break;
                }
                if (asked_again) t_wait += (uint32_t)__builtin_amdgcn_s_memrealtime() - tw0;
                LV<NP> L;
#pragma unroll
                for (int i = 0; i < NP; i++) L.r[i] = want ? (uint32_t)ring[k][i] : border.r[i];
                dg_lds_store<NP>(bufs + (size_t)(r & (DG_RING - 1)) * bufsz + lds_imp, L);
                asm volatile("" ::: "memory");
                if (lane == 0) W[2] = r + 1;                            // (LDS serves one wave's accesses in order: the record is there first)
                fetch(r + DG_AHEAD, ring[k]);
            }
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // (loads of rows past the end still in flight)
    if (lane == 0) W[2] = DG_BIG;                                       // the rows past the end (dead: the trip count is rounded up) never wait
    while (exp_next < ye && !dead) {
        service_exports();
        if (exp_next < ye) {
            __builtin_amdgcn_s_sleep(1);
            give_up();
        }
    }
    if (lane == 0) W[3] = DG_BIG;
    if (lane == 0 && 8 + 8 * strip + 7 < stats_words) {
        int* const st = ctl + 8 + 8 * strip;
        st[0] = (int)t_begin; st[1] = (int)(uint32_t)__builtin_amdgcn_s_memrealtime(); st[2] = spins; st[3] = (int)t_wait; st[4] = misses;
    }
}

// ---- one strip by one workgroup ------------------------------------------------------------------------------------------
template <int NP, bool PAD, int NWC, bool REV, bool WTA>
__device__ __forceinline__ void dg_strip(const DiagJob& job, const SgbmGeom& g, int strip, int nstrips, int* __restrict__ ctl,
                                         int16_t* __restrict__ dump, lds_u8* bufs, lds_u8* scr, lds_vint* W, int stats_words)
{
    constexpr int UW = 4 * NWC, CW = UW + 2;
    const int lane = threadIdx.x & 63, q = lane >> 4, l16 = lane & 15, wv = threadIdx.x >> 6;
    const int W1 = g.W1, H = g.H, Dp = g.Dp;
    const int d0 = l16 * 2 * NP;
    unsigned padreg = 0;
    if constexpr (PAD) {
#pragma unroll
        for (int k = 0; k < NP; k++) padreg |= (unsigned)(d0 + 2 * k >= g.D) << k;
    }
    LV<NP> border;
#pragma unroll
    for (int k = 0; k < NP; k++) border.r[k] = ((padreg >> k) & 1u) ? MAXC2 : 0u;
    const size_t bufsz = (size_t)2 * CW * Dp * 2;
    int ys, ye;
    dg_rows(strip, UW, W1, H, ys, ye);
    // every ring row starts as border everywhere (halo columns included); the progress words start at the strip's first row
    for (int it = threadIdx.x >> 4; it < DG_RING * 2 * CW; it += (NWC + 1) * 4)
        dg_lds_store<NP>(bufs + ((size_t)it * Dp + d0) * 2, border);
    if (threadIdx.x < 2 * NWC + 6) W[threadIdx.x] = threadIdx.x == 2 ? ys - 1 : (threadIdx.x >= 3 && threadIdx.x < 4 + NWC ? ys : (threadIdx.x == 0 ? W[0] : 0));
    dg_barrier();
    if (wv == NWC) {
        dg_helper<NP, NWC>(job, g, strip, nstrips, ctl, bufs, W, padreg, stats_words);
        return;
    }
    constexpr int RPS = NP * 2;                                         // registers per prefetched row
    constexpr int PF = RPS <= 6 ? 6 : RPS <= 8 ? 5 : RPS <= 12 ? 4 : 3;
    const uint32_t P1_2 = pk_rep(g.P1), P2_2 = pk_rep(g.P2);
    const int sc = 4 * wv + q;                                          // this DPP row's column inside the strip
    const int x0 = strip * UW + sc - (H - 1);                           // its pixel at logical row y: x0 + y
    const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)job.C, 0, (int)job.vol_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rI = __builtin_amdgcn_make_buffer_rsrc((void*)job.in1, 0, (int)job.vol_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)(WTA ? (int16_t*)job.C : job.sout), 0, WTA ? 0 : (int)job.vol_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rA0 = __builtin_amdgcn_make_buffer_rsrc((void*)job.aux0, 0, WTA ? (int)job.rec_bytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rA1 = __builtin_amdgcn_make_buffer_rsrc((void*)job.aux1, 0, WTA ? (int)job.rec_bytes : 0, 0x00020000);
    // byte offset of this lane's cells at logical row y (32 bits: a volume has < 2^31 cells).  A pixel outside the image reads
    // the dummy row behind C (cells of P2, i.e. cost 0: it then carries the border state on all three paths by itself --
    // every path that can reach a cell of the image through it, NW from the left of the image, NE from its right, has
    // nothing but outside cells behind it, so L = P2 + min(0, ...) - (0 + P2) = 0 there; what the other paths of an outside
    // cell hold is read by outside cells only) and nothing of the aggregated volume (offset out of range: zeros, never used)
    const uint32_t rstride = (uint32_t)(((REV ? -W1 : W1) + 1) * Dp * 2);             // one row down, one column right
    const uint32_t dummyC = (uint32_t)(((size_t)W1 * H * Dp + d0) * 2);
    auto off32 = [&](int y, bool& ok) -> uint32_t {
        ok = (unsigned)(x0 + y) < (unsigned)W1 && y < ye;
        return (uint32_t)(((REV ? H - 1 - y : y) * W1 + x0 + y) * Dp + d0) * 2u;
    };
    LV<NP> cbuf[PF], ibuf[PF];
#pragma unroll
    for (int k = 0; k < PF; k++) {
        bool ok;
        const uint32_t o = off32(ys + k, ok);
        cbuf[k] = lv_bload_nt<NP>(rC, ok ? o : dummyC);
        ibuf[k] = lv_bload_nt<NP>(rI, ok ? o : DG_OOB);
    }
    uint32_t poff = (uint32_t)(((REV ? H - 1 - (ys + PF) : ys + PF) * W1 + x0 + ys + PF) * Dp + d0) * 2u;   // row ys + PF, unchecked
    // (the loop's first wait is counted against the shorter of its two ways in: pad the way in from here with as many
    // vector-memory instructions as a group of PF rows issues, or every PF-th row would wait with two rows in flight)
#pragma unroll
    for (int k = 0; k < 2 * (PF - 1); k++) __builtin_nontemporal_store(0, (int*)dump + 1024 + 128 + 64 * k + lane);
    const uint32_t lds_own = (uint32_t)(((size_t)sc) * Dp + d0) * 2;                  // + dir * CW * Dp * 2 + ring slot * bufsz
    const uint32_t dirsz = (uint32_t)CW * Dp * 2;
    lds_u8* const myS = scr + (size_t)(threadIdx.x >> 4) * 2 * Dp * 2;              // two rows of S per column (WTA)
    // progress words: the right neighbour's (whose previous row this wave reads: the helper's import count for the last compute
    // wave) and the left neighbour's (who reads this wave's rows: the helper's export count for wave 0)
    lds_vint* const w_right = wv == NWC - 1 ? W + 2 : W + 4 + wv + 1;
    lds_vint* const w_left = wv == 0 ? W + 3 : W + 4 + wv - 1;
    lds_vint* const w_mine = W + 4 + wv;
    const uint32_t a_right = (uint32_t)(size_t)w_right, a_left = (uint32_t)(size_t)w_left, a_dead = (uint32_t)(size_t)(W + 4 + NWC + wv);
    const int spin_limit = job.spin_limit;
    const int left_slack = DG_RING - (wv == 0 ? 1 : 2);                  // row y may overwrite its ring slot once *w_left >= y - left_slack

    LV<NP> Lnw = border;
    uint32_t dnw = P2_2;
    // the winner of the previous row's pixel: its record is written one step late, when its two neighbour costs have come back
    // from LDS -- they serve the sub-pixel fit (k_sgbm_post_rows) and settle the uniqueness test (see wta_count)
    int spar = 0, pkey = 0, pcnt = 0, pT = 0;
    bool plive = false;
    uint32_t paoff = 0;
    uint32_t aoff = (uint32_t)((REV ? H - 1 - ys : ys) * g.W + x0 + ys + g.minX1) * 4u;  // byte offset of the record of this lane's pixel at row ys
    const uint32_t astride = (uint32_t)(((REV ? -g.W : g.W) + 1) * 4);
    int nxt_r = *w_right, nxt_l = *w_left;                              // read one row ahead of their use (they only ever grow)
    auto finish_record = [&]() {
        const int pbest = pkey & 255, pminS = pkey >> 8;
        const int i0 = max(pbest - 1, 0), i1 = min(pbest + 1, Dp - 1);
        const lds_u8* const prevS = myS + (size_t)(spar ^ 1) * Dp * 2;
        const int sm = (int)*(const lds_u16*)(prevS + i0 * 2), sp = (int)*(const lds_u16*)(prevS + i1 * 2);
        // costs below T among the excluded ones: the winner itself and its neighbours where they exist
        const int excl = (int)(pminS < pT) + (int)(pbest > 0 && sm < pT) + (int)(pbest < g.D - 1 && sp < pT);
        const uint32_t so = (plive && l16 == 0) ? paoff : DG_OOB;      // (lanes without a record to write: out of range, dropped)
        // (every sum saturated at 32767: OpenCV's `Sval < minS` never fires from minS = SHRT_MAX, bestDisp stays -1 and the pixel
        //  comes out as (minD - 1) * 16 = INVALID, whatever the uniqueness ratio)
        __builtin_amdgcn_raw_buffer_store_b32((pcnt > excl || pminS >= MAXC) ? -1 : pkey, rA0, so, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32((int)(((uint32_t)sm << 16) | (uint32_t)sp), rA1, so, 0, 0);
    };
    // The unrolled body is straight-line code: no branch may separate a prefetch from its use, or the compiler has to
    // assume the shortest path between them and drains the memory queue every step (s_waitcnt vmcnt(~0)).  The trip count is
    // therefore rounded up to whole groups of PF rows; the surplus rows are dead (border state, stores out of range).
    const int yend = ys + (ye - ys + PF - 1) / PF * PF;
    for (int y0 = ys; y0 < yend; y0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const int y = y0 + k;
            {
                // the right neighbour must have published row y - 1, the left one must be done with the slot row y overwrites
                if (__builtin_amdgcn_readfirstlane(nxt_r) < y) dg_spin(a_right, y, a_dead, spin_limit);
                if (__builtin_amdgcn_readfirstlane(nxt_l) < y - left_slack) dg_spin(a_left, y - left_slack, a_dead, spin_limit);
                nxt_r = *w_right;
                nxt_l = *w_left;
                LV<NP> S = ibuf[k];
                const int x = x0 + y;
                const bool live = (unsigned)x < (unsigned)W1 && y < ye;
                const LV<NP> Cv = cbuf[k];
                const lds_u8* const prev = bufs + (size_t)((y - 1) & (DG_RING - 1)) * bufsz + lds_own;
                lds_u8* const cur = bufs + (size_t)(y & (DG_RING - 1)) * bufsz + lds_own;
                const LV<NP> Lnp = dg_lds_load<NP>(prev + (size_t)1 * Dp * 2);             // L_N of column + 1
                const LV<NP> Lnep = dg_lds_load<NP>(prev + dirsz + (size_t)2 * Dp * 2);    // L_NE of column + 2
                const uint32_t dn = pk_rep_add(row_min_u32(lane_min16<NP>(Lnp)), P2_2);
                const uint32_t dne = pk_rep_add(row_min_u32(lane_min16<NP>(Lnep)), P2_2);
                LV<NP> La = path_step2<NP, PAD>(Cv, Lnw, dnw, P1_2, padreg);
                LV<NP> Lb = path_step2<NP, PAD>(Cv, Lnp, dn, P1_2, padreg);
                LV<NP> Lc = path_step2<NP, PAD>(Cv, Lnep, dne, P1_2, padreg);
                dg_lds_store<NP>(cur, Lb);
                dg_lds_store<NP>(cur + dirsz, Lc);
                asm volatile("" ::: "memory");
                if (lane == 0) *w_mine = y + 1;                         // (LDS serves one wave's accesses in order: the row is there first)
                Lnw = La;
                dnw = pk_rep_add(row_min_u32(lane_min16<NP>(La)), P2_2);
#pragma unroll
                for (int i = 0; i < NP; i++) S.r[i] = pk_add_sat(S.r[i], pk_add_sat(La.r[i], pk_add_sat(Lb.r[i], Lc.r[i])));
                // the row PF steps ahead goes into the registers this step has just finished with -- issued only now, behind
                // a scheduling fence: were the load hoisted above the last use of the old values, the two live ranges would
                // overlap, the loop-carried buffer could not keep its registers, and the copies the register allocator then
                // places on the back edge read every prefetched register (a full s_waitcnt vmcnt drain per group of rows)
                __builtin_amdgcn_sched_barrier(0);
                {
                    const bool ok = (unsigned)(x + PF) < (unsigned)W1 && y + PF < ye;
                    cbuf[k] = lv_bload_nt<NP>(rC, ok ? poff : dummyC);
                    ibuf[k] = lv_bload_nt<NP>(rI, ok ? poff : DG_OOB);
                    poff += rstride;
                }
                if constexpr (WTA) {
                    finish_record();                                    // the previous row's pixel
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
                } else {
                    // (this row's cells: the offset the prefetch PF steps ago used, kept in step with it)
                    lv_bstore_nt<NP>(rO, live ? poff - (uint32_t)(PF + 1) * rstride : DG_OOB, S);
                }
            }
        }
    }
    if (lane == 0) *w_mine = DG_BIG;                                    // nobody waits for a wave that has left
    if constexpr (WTA) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        finish_record();
    }
    if (__builtin_amdgcn_readfirstlane(*(lds_vint*)(W + 4 + NWC + wv)) && lane == 0) atomicExch(job.ctl + 1, 1);   // this wave gave up a wait
}

// persistent workgroups: (pair, strip) work items off a ticket counter, right-most strip of a pair first
template <int NP, bool PAD, int NWC, bool REV, bool WTA>
__global__ void __launch_bounds__((NWC + 1) * 64, NP <= 4 ? 4 : 2) k_sgbm_diag(DiagJobs jobs, SgbmGeom g, int* __restrict__ ctl, int16_t* __restrict__ dump, int stats_words)
{
    constexpr int UW = 4 * NWC, CW = UW + 2;
    extern __shared__ u32x4 s_dg[];
    lds_u8* const bufs = (lds_u8*)s_dg;                                                  // [DG_RING][2][CW][Dp] int16
    lds_u8* const scr = bufs + (size_t)DG_RING * 2 * CW * g.Dp * 2;                      // [NWC * 4][2][Dp] int16 (WTA)
    lds_vint* const words = (lds_vint*)(scr + (WTA ? (size_t)NWC * 4 * 2 * g.Dp * 2 : 0));   // control words (see DG_RING)
    const int total = jobs.n * jobs.nstrips;
    for (;;) {
        __syncthreads();                                                                // everybody is done with the previous strip's LDS
        if (threadIdx.x == 0) words[0] = atomicAdd(ctl, 1);
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(words[0]);
        if (t >= total) return;
        // pairs interleaved: the n pairs of a launch advance side by side, each over its own right-most strips first (a strip
        // still only waits for strips of its own pair with lower tickets)
        const int k = t / jobs.n, pair = t - k * jobs.n, strip = jobs.nstrips - 1 - k;
        dg_strip<NP, PAD, NWC, REV, WTA>(jobs.j[pair], g, strip, jobs.nstrips, ctl, dump, bufs, scr, words, pair == 0 ? stats_words : 0);
    }
}
