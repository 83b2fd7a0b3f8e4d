// Brute-force Hamming kNN (k = 2) on gfx950: replaces
// self.matcher.knnMatch(desc1, desc2, k=2) with cv2.NORM_HAMMING [reference stereo_odometer.py:22,163].
// Ordering rule of OpenCV's batch_distance.cpp: ascending distance, ties -> lower train index,
// which is exactly the lexicographic minimum of (distance, trainIdx).
//
//
// Round 5: the distance table as an integer-exact dense contraction on the matrix cores.  popcount(q ^ t) = |q| + |t| - 2 q.t
// over {0,1} vectors, and q.t over 256 bits is four v_mfma_i32_16x16x64_i8 on bits expanded to bytes -- exact in int32 (the
// one stage of this path that IS a dense contraction: 8000 x 8000 x 256 bit = 1.6e10 multiply-adds at config 5).
//   * a wave owns 64 queries (four 16-row A operands, expanded once into 64 registers) and walks a slice of the train set in
//     tiles of 16 descriptors.  Bits become bytes by v_bfe, v_mul_u32_u24 by 0x204081, v_and (a nibble -> four bytes); the
//     queries' bytes are {0, -1} so that the accumulators hold -(q.t).  The eight waves of a workgroup share ONE expanded copy
//     of their slice in LDS (32 tiles = 128 KB at a time): per tile a wave issues four ds_read_b128, sixteen MFMAs, and per
//     accumulator register key = ((|t| + 256) << 16 | j) + (-(q.t) << 17) (one v_lshl_add_u32) and a
//     private best / second (v_med3_u32, v_min_u32).  |q| is the same for every candidate of a query, so it is added when the
//     result is written.  The k order inside the MFMA is irrelevant: both operands cut a descriptor the same way (lane group
//     g = lane >> 4 takes bits 64 g .. 64 g + 63, MFMA m its m-th 16), and a dot product does not care in which order it sums.
//   * key order = (distance, train index) lexicographic = batch_distance.cpp's "ascending, ties to the lower index".
//   * a query's candidates sit in the 16 lanes of a DPP row (the C layout puts the train on lane & 15): four row_ror butterfly
//     steps merge the private pairs once per wave.
//   * the train set is cut into up to 16 slices (about 2000 waves at 8000 x 8000: two per SIMD); a slice's pairs go to scratch
//     behind the distances, the wave that draws a group's last ticket merges them (agent-scope release / acquire around the
//     ticket) and writes idx / dist.  One launch; 4 MB of L2 traffic at config 5 (every workgroup reads its slice once).
//   * k_bf_knn2<true> (cross-check, DESIGN 4d'): the same tiles also give every train descriptor its nearest query (column minima:
//     16 keys per lane -> permlane swaps across the four lane groups -> ds_min across the waves -> one global atomicMin per train
//     descriptor and LDS chunk).  k_bf_knn2<false> is the kernel above, instruction for instruction.
#include "vo_internal.h"

typedef int v4i __attribute__((ext_vector_type(4)));

// bits 4 i .. 4 i + 3 of x -> four bytes of {0, 1} (bit k of the nibble in byte k)
#define NIB(x, i) ((__umul24(__builtin_amdgcn_ubfe((x), 4 * (i), 4), 0x00204081u)) & 0x01010101u)
__device__ __forceinline__ void expand64(uint32_t lo, uint32_t hi, v4i (&o)[4])
{
    o[0] = (v4i){ (int)NIB(lo, 0), (int)NIB(lo, 1), (int)NIB(lo, 2), (int)NIB(lo, 3) };
    o[1] = (v4i){ (int)NIB(lo, 4), (int)NIB(lo, 5), (int)NIB(lo, 6), (int)NIB(lo, 7) };
    o[2] = (v4i){ (int)NIB(hi, 0), (int)NIB(hi, 1), (int)NIB(hi, 2), (int)NIB(hi, 3) };
    o[3] = (v4i){ (int)NIB(hi, 4), (int)NIB(hi, 5), (int)NIB(hi, 6), (int)NIB(hi, 7) };
}
#undef NIB

__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// (a0 <= a1) and (b0 <= b1) -> the two smallest of the four
__device__ __forceinline__ void merge2(uint32_t& a0, uint32_t& a1, uint32_t b0, uint32_t b1)
{
    const uint32_t hi = max(a0, b0);
    a0 = min(a0, b0);
    a1 = min(hi, min(a1, b1));
}

#define KNN_NONE 0x70000000u     // keys at or above: no such neighbour (valid keys stay below 0x03010000)

#define KNN_WAVES 8              // waves (= groups of 64 queries) per workgroup: they share one slice of the train set in LDS
#define KNN_CHUNK 32            // tiles of 16 train descriptors expanded into LDS at a time: 32 x 4 KB + their bit counts = 130 KB
// WINDOW (DESIGN 4d''): train j is a candidate of query i only if |xq_i - xt_j| <= rx and |yq_i - yt_j| <= ry (float32, NaN in no
// window); every other element's key is 0xFFFFFFFF, in the row state and in the column minimum alike.  A tile of 16 trains whose
// bounding box cannot reach the bounding box of the wave's 64 queries is skipped before its LDS reads and MFMAs.
#define ROW_ROR_F(v, c) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x120 + (c), 0xf, 0xf, false))
template <bool CROSS, bool WINDOW>
__global__ void __launch_bounds__(KNN_WAVES * 64) k_bf_knn2(const uint8_t* __restrict__ q, int nq, const uint8_t* __restrict__ t, int nt, int splits,
                                               int tiles_per_split, int ngroups, unsigned long long* __restrict__ part, int* __restrict__ tickets,
                                               int32_t* __restrict__ idx, int32_t* __restrict__ dist, uint32_t* __restrict__ colmin,
                                               const float2* __restrict__ xy_q, const float2* __restrict__ xy_t, float rx, float ry)
{
    const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int gblock = blockIdx.x / splits, split = blockIdx.x - gblock * splits;
    const int group = gblock * KNN_WAVES + (threadIdx.x >> 6);
    const int q0 = group * 64, nqp = ngroups * 64;
    const int ntiles = (nt + 15) >> 4;
    const int t0 = split * tiles_per_split, t1 = min(ntiles, t0 + tiles_per_split);
    const bool active = group < ngroups;                  // (a wave past the last group of queries only helps to fill the LDS)

    // The slice of the train set this workgroup walks is EXPANDED into LDS, a chunk of KNN_CHUNK tiles at a time, by all waves
    // together: the B operand of MFMA m of tile T for lane (col, g) = the 16 bytes made of bits 64 g + 16 m .. + 15 of train
    // 16 T + col, at ((T * 4 + m) * 64 + lane) * 16 -- a wave's ds_read_b128 covers 1 KB contiguously.  The expansion (three
    // vector instructions per four bits) is thereby paid once per workgroup instead of once per wave, and the tile loop never
    // waits for global memory.
    extern __shared__ uint4 s_lds4[];
    const int chunk_tiles = min(KNN_CHUNK, max(1, tiles_per_split));
    uint4* const s_B = s_lds4;                                           // [chunk_tiles][4][64]
    int* const s_tn = (int*)(s_lds4 + (size_t)chunk_tiles * 256);        // [chunk_tiles * 16]: |t| + 256, or 0x7FFF past the end
    uint32_t* const s_col = (uint32_t*)(s_tn + chunk_tiles * 16);         // CROSS: [chunk_tiles * 16] column minima of the chunk
    float2* const s_txy = (float2*)(s_col + (CROSS ? chunk_tiles * 16 : 0));   // WINDOW: [chunk_tiles * 16] train positions (NaN past the end)
    float4* const s_box = (float4*)(s_txy + chunk_tiles * 16);            // WINDOW: [chunk_tiles] {min x, max x, min y, max y} of a tile's trains

    v4i A[4][4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int qi = max(0, min(q0 + 16 * s + col, nq - 1));
        const uint2 w = *(const uint2*)(q + (size_t)qi * 32 + 8 * g);
        expand64(w.x, w.y, A[s]);
#pragma unroll
        for (int m = 0; m < 4; m++) A[s][m] *= 0xFF;      // bytes of {0, -1}: the accumulators hold -(q.t), and the key below is ONE v_lshl_add_u32
    }
    // CROSS: the column key of accumulator register r of sub-tile s is cb[s][r] + (-(q.t) << 17) = ((|q| - 2 q.t + 256) << 16) | query
    // for query 16 s + 4 g + r of the wave (|t| is the same for every candidate of a train column and is added at the decode).
    // Rows past nq repeat query nq - 1 (as the A operands do) under ITS index: an exact copy of a key that is present anyway.
    uint32_t cb[4][4];
    if constexpr (CROSS) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int qi = max(0, min(q0 + 16 * s + 4 * g + r, nq - 1));
                const uint4* qp = (const uint4*)(q + (size_t)qi * 32);
                const uint4 a = qp[0], b = qp[1];
                const int qn = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
                cb[s][r] = ((uint32_t)(qn + 256) << 16) | (uint32_t)qi;
            }
    }
    uint32_t k0[4][4], k1[4][4];
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int r = 0; r < 4; r++) k0[s][r] = k1[s][r] = 0xFFFFFFFFu;
    // WINDOW: the position of query 16 s + 4 g + r, the row that k0[s][r] belongs to (rows past nq repeat query nq - 1 with ITS
    // position), and the bounding box of the wave's 64 queries (a NaN coordinate is in no window and in no box)
    float2 pq[4][4];
    float qx0 = __builtin_inff(), qx1 = -__builtin_inff(), qy0 = __builtin_inff(), qy1 = -__builtin_inff();
    if constexpr (WINDOW) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float2 p = xy_q[max(0, min(q0 + 16 * s + 4 * g + r, nq - 1))];
                pq[s][r] = p;
                if (p.x == p.x) { qx0 = fminf(qx0, p.x); qx1 = fmaxf(qx1, p.x); }
                if (p.y == p.y) { qy0 = fminf(qy0, p.y); qy1 = fmaxf(qy1, p.y); }
            }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {               // the four lane groups hold 16 queries each
            qx0 = fminf(qx0, __shfl_xor(qx0, o, 64)); qx1 = fmaxf(qx1, __shfl_xor(qx1, o, 64));
            qy0 = fminf(qy0, __shfl_xor(qy0, o, 64)); qy1 = fmaxf(qy1, __shfl_xor(qy1, o, 64));
        }
    }

    for (int c0 = t0; c0 < t1; c0 += KNN_CHUNK) {
        const int c1 = min(t1, c0 + KNN_CHUNK);
        if (c0 != t0) __syncthreads();                    // (every wave is done with the previous chunk)
        if constexpr (CROSS) {
            // the previous chunk's column minima go out (one global atomic per train descriptor), the words start over
            if (threadIdx.x < chunk_tiles * 16) {
                if (c0 != t0) {
                    const int j = (c0 - KNN_CHUNK) * 16 + threadIdx.x;
                    if (j < nt) __hip_atomic_fetch_min(colmin + j, s_col[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                s_col[threadIdx.x] = 0xFFFFFFFFu;
            }
        }
        for (int i = threadIdx.x; i < (c1 - c0) * 16; i += KNN_WAVES * 64) {     // one train descriptor per thread
            const int j = c0 * 16 + i;
            uint4 a = make_uint4(0, 0, 0, 0), b = a;
            if (j < nt) {
                const uint4* tp = (const uint4*)(t + (size_t)j * 32);
                a = tp[0]; b = tp[1];
            }
            uint4* const dst = s_B + (size_t)(i >> 4) * 256 + (i & 15);          // + m * 64 + g * 16
            const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                v4i e[4];
                expand64(w[2 * gg], w[2 * gg + 1], e);
#pragma unroll
                for (int m = 0; m < 4; m++) dst[m * 64 + gg * 16] = make_uint4((uint32_t)e[m].x, (uint32_t)e[m].y, (uint32_t)e[m].z, (uint32_t)e[m].w);
            }
            s_tn[i] = j < nt ? __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w) + 256 : 0x7FFF;
            if constexpr (WINDOW) {
                // the 16 trains of a tile sit in one DPP row (i and the trip count are multiples of 16 apart: a row is whole or idle)
                const float nan = __builtin_nanf("");
                const float2 p = j < nt ? xy_t[j] : make_float2(nan, nan);
                s_txy[i] = p;
                float x0 = p.x == p.x ? p.x : __builtin_inff(), x1 = p.x == p.x ? p.x : -__builtin_inff();
                float y0 = p.y == p.y ? p.y : __builtin_inff(), y1 = p.y == p.y ? p.y : -__builtin_inff();
#define ROW_BOX(c) x0 = fminf(x0, ROW_ROR_F(x0, c)); x1 = fmaxf(x1, ROW_ROR_F(x1, c)); y0 = fminf(y0, ROW_ROR_F(y0, c)); y1 = fmaxf(y1, ROW_ROR_F(y1, c));
                ROW_BOX(8) ROW_BOX(4) ROW_BOX(2) ROW_BOX(1)
#undef ROW_BOX
                if ((i & 15) == 0) s_box[i >> 4] = make_float4(x0, x1, y0, y1);
            }
        }
        __syncthreads();
        if (!active) continue;
        const uint4* const s_w = s_B + lane;
        const int* const s_n = s_tn + col;
        if constexpr (WINDOW) {
            // One bit per tile of the chunk whose box can reach the wave's box (lane L tests tile c0 + L; a ballot is wave-uniform).
            // Conservative under rounding: float subtraction is monotone, so fl(min - max) > r implies |xq - xt| > r for every
            // pair drawn from the two boxes.  An empty box is (+inf, -inf): unreachable.
            bool reach = false;
            if (lane < c1 - c0) {
                const float4 bx = s_box[lane];
                reach = !(bx.x - qx1 > rx || qx0 - bx.y > rx || bx.z - qy1 > ry || qy0 - bx.w > ry);
            }
            uint32_t todo = (uint32_t)__ballot(reach);
            while (todo) {
                const int tl = __builtin_ctz(todo);          // tile c0 + tl
                todo &= todo - 1;
                v4i B[4];
#pragma unroll
                for (int m = 0; m < 4; m++) { const uint4 u = s_w[tl * 256 + m * 64]; B[m] = (v4i){ (int)u.x, (int)u.y, (int)u.z, (int)u.w }; }
                const int tn = s_n[tl * 16];                 // |t| + 256, or 0x7FFF past the end of the train set (its position is NaN)
                const float2 pt = s_txy[tl * 16 + col];
                const uint32_t base = ((uint32_t)tn << 16) | (uint32_t)(((c0 + tl) * 16 + col) & 0xFFFF);
                uint32_t cm = 0xFFFFFFFFu;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    v4i acc = { 0, 0, 0, 0 };
#pragma unroll
                    for (int m = 0; m < 4; m++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[s][m], B[m], acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const bool in = fabsf(pq[s][r].x - pt.x) <= rx && fabsf(pq[s][r].y - pt.y) <= ry;
                        const uint32_t key = in ? base + ((uint32_t)acc[r] << 17) : 0xFFFFFFFFu;
                        k1[s][r] = med3_u32(k0[s][r], k1[s][r], key);
                        k0[s][r] = min(k0[s][r], key);
                        if constexpr (CROSS) cm = min(cm, in ? cb[s][r] + ((uint32_t)acc[r] << 17) : 0xFFFFFFFFu);
                    }
                }
                if constexpr (CROSS) {
                    const auto x = __builtin_amdgcn_permlane32_swap(cm, cm, false, false);
                    cm = min(x[0], x[1]);
                    const auto y = __builtin_amdgcn_permlane16_swap(cm, cm, false, false);
                    cm = min(y[0], y[1]);
                    if (lane < 16) atomicMin(s_col + tl * 16 + col, cm);
                }
            }
            continue;
        }
        v4i Bn[4];
#pragma unroll
        for (int m = 0; m < 4; m++) { const uint4 u = s_w[m * 64]; Bn[m] = (v4i){ (int)u.x, (int)u.y, (int)u.z, (int)u.w }; }
        int tn_nxt = s_n[0];
        for (int tile = c0; tile < c1; tile++) {
            v4i B[4];
#pragma unroll
            for (int m = 0; m < 4; m++) B[m] = Bn[m];
            const int tn = tn_nxt;                       // |t| + 256, or 0x7FFF past the end of the train set: never a winner
            if (tile + 1 < c1) {
#pragma unroll
                for (int m = 0; m < 4; m++) { const uint4 u = s_w[(tile + 1 - c0) * 256 + m * 64]; Bn[m] = (v4i){ (int)u.x, (int)u.y, (int)u.z, (int)u.w }; }
                tn_nxt = s_n[(tile + 1 - c0) * 16];
            }
            const uint32_t base = ((uint32_t)tn << 16) | (uint32_t)((tile * 16 + col) & 0xFFFF);
            uint32_t cm = 0xFFFFFFFFu;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                v4i acc = { 0, 0, 0, 0 };
#pragma unroll
                for (int m = 0; m < 4; m++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[s][m], B[m], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    // base - (q.t << 17): row 4 g + r of sub-tile s against train j.  Plain C on purpose: an inline-asm instruction
                    // that reads an MFMA result gets none of the wait states the compiler pads its own instructions with
                    // (measured: short sums)
                    const uint32_t key = base + ((uint32_t)acc[r] << 17);
                    k1[s][r] = med3_u32(k0[s][r], k1[s][r], key);
                    k0[s][r] = min(k0[s][r], key);
                    if constexpr (CROSS) cm = min(cm, cb[s][r] + ((uint32_t)acc[r] << 17));
                }
            }
            if constexpr (CROSS) {
                // the 16 keys of train 16 tile + col this lane holds -> the four lane groups (rows of 16 lanes) -> every wave
                const auto x = __builtin_amdgcn_permlane32_swap(cm, cm, false, false);     // rows 0 1 | 2 3
                cm = min(x[0], x[1]);
                const auto y = __builtin_amdgcn_permlane16_swap(cm, cm, false, false);     // rows 0 | 1
                cm = min(y[0], y[1]);
                if (lane < 16) atomicMin(s_col + (tile - c0) * 16 + col, cm);
            }
        }
    }
    if constexpr (CROSS) {
        __syncthreads();                                  // (every wave is done with the last chunk)
        if (t1 > t0 && threadIdx.x < chunk_tiles * 16) {
            const int j = (t0 + (t1 - t0 - 1) / KNN_CHUNK * KNN_CHUNK) * 16 + threadIdx.x;
            if (j < nt && j < t1 * 16) __hip_atomic_fetch_min(colmin + j, s_col[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!active) return;
    // the 16 lanes of a DPP row hold disjoint candidate sets of the same four queries: butterfly (row_ror 8, 4, 2, 1)
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t a0 = k0[s][r], a1 = k1[s][r];
#define ROR(v, c) (uint32_t)__builtin_amdgcn_update_dpp((int)(v), (int)(v), 0x120 + (c), 0xf, 0xf, false)
            merge2(a0, a1, ROR(a0, 8), ROR(a1, 8));
            merge2(a0, a1, ROR(a0, 4), ROR(a1, 4));
            merge2(a0, a1, ROR(a0, 2), ROR(a1, 2));
            merge2(a0, a1, ROR(a0, 1), ROR(a1, 1));
#undef ROR
            if (col == 4 * s + r)                       // one lane per (group of rows, state): query 16 s + 4 g + r
                __hip_atomic_store(part + (size_t)split * nqp + q0 + 16 * s + 4 * g + r, (unsigned long long)a0 | ((unsigned long long)a1 << 32),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // write-through (sc1): see the ticket below
        }
    // ticket: the wave that finishes a group's last slice merges the slices (its own included) and writes the result
    // Hand-off without fences (MI355X_MICROARCH.md, inter-workgroup visibility: sc1 stores -> the storing wave's vmcnt(0) -> ONE
    // agent-scope add by one lane -> the wave whose add came last reads with sc1 loads after its add has returned).  An
    // agent-scope release fence instead writes back the XCD's whole L2 (1.7 - 6.5 us each, and 2000 waves would each pay it).
    int last = 1;
    if (splits > 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int tk = 0;
        if (lane == 0) tk = __hip_atomic_fetch_add(tickets + group, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        last = tk == splits - 1;
    }
    if (!last) return;
    if (splits > 1 && lane == 0) __hip_atomic_store(tickets + group, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch finds it cleared
    const int qi = q0 + lane;
    if (qi >= nq) return;
    uint32_t a0 = 0xFFFFFFFFu, a1 = 0xFFFFFFFFu;
    unsigned long long p[VO_KNN_SPLITS];             // every slice's pair in flight at once (one after the other: 16 x the latency)
#pragma unroll
    for (int s = 0; s < VO_KNN_SPLITS; s++)
        p[s] = __hip_atomic_load(part + (size_t)(s < splits ? s : 0) * nqp + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (no branch: slice 0 again)
#pragma unroll
    for (int s = 0; s < VO_KNN_SPLITS; s++)
        if (s < splits) merge2(a0, a1, (uint32_t)p[s], (uint32_t)(p[s] >> 32));
    const uint4* qp = (const uint4*)(q + (size_t)qi * 32);
    const uint4 qa = qp[0], qb = qp[1];
    const int qn = __popc(qa.x) + __popc(qa.y) + __popc(qa.z) + __popc(qa.w) + __popc(qb.x) + __popc(qb.y) + __popc(qb.z) + __popc(qb.w);
    const bool h0 = a0 < KNN_NONE, h1 = a1 < KNN_NONE;
    idx[2 * qi] = h0 ? (int32_t)(a0 & 0xFFFFu) : -1;
    dist[2 * qi] = h0 ? (int32_t)(a0 >> 16) - 256 + qn : 0x7FFFFFFF;
    idx[2 * qi + 1] = h1 ? (int32_t)(a1 & 0xFFFFu) : -1;
    dist[2 * qi + 1] = h1 ? (int32_t)(a1 >> 16) - 256 + qn : 0x7FFFFFFF;
}

hipError_t match_ws_alloc(vo_ctx* ctx, vo_ctx::MatchWs& m, int what)
{
    const size_t cap = (size_t)ctx->kp_cap, dist = match_dist_bytes(ctx->kp_cap), clique = pose_ws_bytes(ctx->kp_cap);
    const bool pose = (what & MATCH_WS_POSE) != 0;
    const struct { void** p; size_t bytes; bool take; } tab[] = {
        { (void**)&m.m_idx, cap * 8 + 256, true },   { (void**)&m.m_dist, dist, true },         { (void**)&m.m_count, 512, true },
        { (void**)&m.mq_idx, cap * 4 + 256, true },  { (void**)&m.mt_idx, cap * 4 + 256, true },
        { (void**)&m.xy_a, cap * 8 + 256, true },    { (void**)&m.xy_b, cap * 8 + 256, true },
        { (void**)&m.pts_a, cap * 12 + 256, pose },  { (void**)&m.pts_b, cap * 12 + 256, pose },
        { (void**)&m.st_a, cap + 256, pose },        { (void**)&m.st_b, cap + 256, pose },
        { (void**)&m.clique_ws, clique + 256, pose },            // sized once: the pose step never reallocates mid-stream
    };
    hipError_t e = hipSuccess;
    for (const auto& t : tab)
        if (t.take && e == hipSuccess) e = hipMalloc(t.p, t.bytes);
    // (the kNN tickets inside m_dist must read zero before the first launch, on whatever stream that is)
    if (e == hipSuccess) e = dev_zero(m.m_dist, dist);
    if (e != hipSuccess) { match_ws_free(m); return e; }
    if (pose) m.clique_ws_bytes = clique;
    return hipSuccess;
}

int ws_reserve(vo_ctx* ctx, uint8_t** ptr, size_t* bytes, size_t need, size_t floor)
{
    if (*bytes >= need) return VO_OK;
    VO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (work in flight may still use the old buffer)
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr; *bytes = 0;
    const size_t take = need > floor ? need : floor;
    VO_HIP(ctx, hipMalloc((void**)ptr, take));
    *bytes = take;
    return VO_OK;
}

void match_ws_free(vo_ctx::MatchWs& m)
{
    void* ps[] = { m.m_idx, m.m_dist, m.m_count, m.mq_idx, m.mt_idx, m.xy_a, m.xy_b, m.pts_a, m.pts_b, m.st_a, m.st_b, m.clique_ws, m.ransac_ws };
    for (void* q : ps) if (q) (void)hipFree(q);
    klt_ws_free(m.klt);
    m = vo_ctx::MatchWs();
}

// d_dist must be an allocation of match_dist_bytes(kp_cap): the distances, then the slices' partial pairs, then the tickets
// (zeroed once by match_ws_alloc; every launch leaves them zero), then the per-train column words of the cross-check.
// cross != 0: the same launch also leaves, for every train descriptor j, the key of its nearest query in match_colmin(d_dist)
// (reset on the launching stream first; read by the consumers of the next launches, never inside this one)
// xy_q / xy_t (both or neither; nullptr = no window): the keypoint positions behind the descriptors, nq and nt float pairs in
// device memory; the windowed kernel then takes the radii by value (a launch keeps the window it was enqueued with)
int match_knn2(vo_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int32_t* d_idx, int32_t* d_dist, int cross, const float* xy_q,
               const float* xy_t, float rx, float ry)
{
    const bool window = xy_q != nullptr;
    if (window && (!xy_t || !(rx >= 0.f) || !(ry >= 0.f) || rx > 3.4028234e38f || ry > 3.4028234e38f))
        return vo_fail(ctx, VO_E_ARG, "windowed kNN: needs both position arrays and finite radii >= 0");
    if (nt > 65535) return vo_fail(ctx, VO_E_CAP, "train set of %d descriptors exceeds 65535", nt);
    if (cross && nq > 65535) return vo_fail(ctx, VO_E_CAP, "cross-check: query set of %d descriptors exceeds 65535", nq);
    if (cross && nt > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "cross-check: train set of %d descriptors exceeds capacity %d", nt, ctx->kp_cap);
    if (nq <= 0) return VO_OK;
    if (nq > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "query set of %d descriptors exceeds capacity %d", nq, ctx->kp_cap);
    const int groups = div_up(nq, 64), gblocks = div_up(groups, KNN_WAVES), ntiles = div_up(nt, 16);
    // about 2000 waves (two per SIMD), a slice of at least 2 tiles, at most VO_KNN_SPLITS slices
    int splits = std::min(std::min(VO_KNN_SPLITS, std::max(1, ntiles / 2)), div_up(2048, gblocks * KNN_WAVES));
    const int per = std::max(1, div_up(ntiles, splits));
    splits = std::max(1, div_up(ntiles, per));
    const size_t capq = ((size_t)ctx->kp_cap + 63) & ~(size_t)63;
    unsigned long long* part = (unsigned long long*)(d_dist + 2 * capq);
    int* tickets = (int*)(part + (size_t)VO_KNN_SPLITS * capq);
    uint32_t* colmin = cross ? match_colmin(d_dist, ctx->kp_cap) : nullptr;
    // per train: the expanded descriptor, its bit count (+ a column word) (+ its position); WINDOW: one box per tile behind them
    const size_t lds = (size_t)std::min(per, KNN_CHUNK) * (16 * (256 + 4 + (cross ? 4 : 0) + (window ? 8 : 0)) + (window ? 16 : 0));
    auto kern = window ? (cross ? k_bf_knn2<true, true> : k_bf_knn2<false, true>) : (cross ? k_bf_knn2<true, false> : k_bf_knn2<false, false>);
    if (lds > 64 * 1024)
        if (int rca = lds_allow_big(ctx, (const void*)kern)) return rca;
    // (the column words are reset on the stream that launches: a null-stream memset does not order itself against the
    // alternates' streams)
    if (cross && nt > 0) VO_HIP(ctx, hipMemsetAsync(colmin, 0xFF, (size_t)nt * 4, ctx->stream));
    StageTimer tk(ctx, VO_T_KNN);
    hipLaunchKernelGGL(kern, dim3(gblocks * splits), dim3(KNN_WAVES * 64), lds, ctx->stream, dq, nq, dt, nt, splits, per, groups, part, tickets, d_idx,
                       d_dist, colmin, (const float2*)xy_q, (const float2*)xy_t, rx, ry);
    VO_CHECK_LAUNCH(ctx);
    return VO_OK;
}

extern "C" int vo_set_match_window(vo_ctx* ctx, float rx, float ry)
{
    if (!ctx) return VO_E_ARG;
    if (!(rx >= 0.f) || !(ry >= 0.f) || rx > 3.4028234e38f || ry > 3.4028234e38f)
        return vo_fail(ctx, VO_E_ARG, "vo_set_match_window: the radii must be finite and >= 0");
    ctx->has_win = true; ctx->win_rx = rx; ctx->win_ry = ry;
    return VO_OK;
}

extern "C" int vo_clear_match_window(vo_ctx* ctx)
{
    if (!ctx) return VO_E_ARG;
    if (!ctx->has_win) return vo_fail(ctx, VO_E_STATE, "vo_clear_match_window: no window is set");
    ctx->has_win = false; ctx->win_rx = ctx->win_ry = 0.f;
    return VO_OK;
}

extern "C" int vo_set_match_loop(vo_ctx* ctx, int max_hamming)
{
    if (!ctx) return VO_E_ARG;
    if (max_hamming < 0 || max_hamming > 256) return vo_fail(ctx, VO_E_ARG, "vo_set_match_loop: max_hamming is 0 .. 256");
    ctx->has_loop = true; ctx->loop_max = max_hamming;
    return VO_OK;
}

extern "C" int vo_clear_match_loop(vo_ctx* ctx)
{
    if (!ctx) return VO_E_ARG;
    if (!ctx->has_loop) return vo_fail(ctx, VO_E_STATE, "vo_clear_match_loop: no threshold is set");
    ctx->has_loop = false; ctx->loop_max = 0;
    return VO_OK;
}

int match_loop_gate(vo_ctx* ctx, const FrameSlot& a, const FrameSlot& b, int match_flags, const char* who, LoopGate* g)
{
    *g = LoopGate();
    if (!(match_flags & VO_MATCH_LOOP)) return VO_OK;      // (match_flags_check has passed: a threshold is set)
    if (!slot_sparse(a) || !slot_sparse(b))
        return vo_fail(ctx, VO_E_STATE, "%s: VO_MATCH_LOOP needs both slots' keypoints to carry depth (vo_sparse_stereo)", who);
    g->rd_a = a.kp_rdesc; g->rd_b = b.kp_rdesc; g->max_h = ctx->loop_max;
    return VO_OK;
}

int match_flags_check(vo_ctx* ctx, int match_flags, const char* who, bool loop_ok)
{
    if (match_flags & ~(VO_MATCH_CROSSCHECK | VO_MATCH_WINDOW | VO_MATCH_LOOP)) return vo_fail(ctx, VO_E_ARG, "%s: bad argument (unknown match_flags bits)", who);
    if (match_flags & VO_MATCH_LOOP) {
        if (!loop_ok) return vo_fail(ctx, VO_E_ARG, "%s: VO_MATCH_LOOP belongs to the stereo pair steps on sparse slots", who);
        if (!ctx->has_loop) return vo_fail(ctx, VO_E_ARG, "%s: VO_MATCH_LOOP without a threshold (call vo_set_match_loop first)", who);
    }
    if ((match_flags & VO_MATCH_WINDOW) && !ctx->has_win)
        return vo_fail(ctx, VO_E_ARG, "%s: VO_MATCH_WINDOW without a window (call vo_set_match_window first)", who);
    return VO_OK;
}

int match_knn2_slots(vo_ctx* ctx, const FrameSlot& a, const FrameSlot& b, int match_flags)
{
    if (int rc = match_flags_check(ctx, match_flags, "kNN of two slots", true)) return rc;     // (the loop check is the prep kernel's business)
    const bool window = (match_flags & VO_MATCH_WINDOW) != 0;
    return match_knn2(ctx, a.desc, a.n_kp, b.desc, b.n_kp, ctx->mw->m_idx, ctx->mw->m_dist, match_flags & VO_MATCH_CROSSCHECK,
                      window ? a.kp_xy : nullptr, window ? b.kp_xy : nullptr, ctx->win_rx, ctx->win_ry);
}

extern "C" int vo_measure_knn_ex(vo_ctx* ctx, int slot_a, int slot_b, int reps, int match_flags, double* us_per_launch)
{
    if (!ctx || !us_per_launch || reps <= 0 || reps > 10000 || slot_a < 0 || slot_a >= VO_NUM_SLOTS || slot_b < 0 || slot_b >= VO_NUM_SLOTS)
        return vo_fail(ctx, VO_E_ARG, "vo_measure_knn: bad argument");
    if (int rcf = match_flags_check(ctx, match_flags, "vo_measure_knn")) return rcf;
    FrameSlot& a = ctx->slots[slot_a];
    FrameSlot& b = ctx->slots[slot_b];
    if (!a.has_kp || !b.has_kp || a.n_kp <= 0) return vo_fail(ctx, VO_E_STATE, "vo_measure_knn: both slots need keypoints");
    VO_HIP(ctx, hipSetDevice(ctx->device));
    { int rcw = slot_wait(ctx, a); if (!rcw) rcw = slot_wait(ctx, b); if (rcw) return rcw; }
    hipEvent_t e0, e1;
    VO_HIP(ctx, hipEventCreate(&e0));
    VO_HIP(ctx, hipEventCreate(&e1));
    int rc = match_knn2_slots(ctx, a, b, match_flags);      // warm-up (LDS attribute, caches)
    if (!rc && hipEventRecord(e0, ctx->stream) != hipSuccess) rc = VO_E_HIP;
    for (int r = 0; r < reps && !rc; r++) rc = match_knn2_slots(ctx, a, b, match_flags);
    if (!rc && hipEventRecord(e1, ctx->stream) != hipSuccess) rc = VO_E_HIP;
    float ms = 0.f;
    if (!rc && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) rc = VO_E_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc == VO_E_HIP ? vo_fail(ctx, VO_E_HIP, "vo_measure_knn: HIP error") : rc;
    *us_per_launch = 1e3 * (double)ms / reps;
    return VO_OK;
}

extern "C" int vo_measure_knn(vo_ctx* ctx, int slot_a, int slot_b, int reps, double* us_per_launch)
{
    return vo_measure_knn_ex(ctx, slot_a, slot_b, reps, 0, us_per_launch);
}

extern "C" int vo_bf_knn2_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx,
                                  int32_t* dist)
{
    if (!ctx || nq < 0 || nt < 0 || (nq && (!q || !idx || !dist)) || (nt && !t)) return vo_fail(ctx, VO_E_ARG, "vo_bf_knn2_hamming: bad argument");
    if (nq > ctx->kp_cap || nt > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "descriptor count exceeds capacity %d", ctx->kp_cap);
    if (nq == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    StageTimer tm(ctx, VO_T_MATCH);
    int rc = xfer_h2d(ctx, ctx->mq, q, (size_t)nq * 32);
    if (!rc && nt) rc = xfer_h2d(ctx, ctx->mt, t, (size_t)nt * 32);
    if (rc) return rc;
    rc = match_knn2(ctx, ctx->mq, nq, ctx->mt, nt, ctx->mw->m_idx, ctx->mw->m_dist);
    if (rc) return rc;
    rc = xfer_d2h(ctx, idx, ctx->mw->m_idx, (size_t)nq * 8);
    if (!rc) rc = xfer_d2h(ctx, dist, ctx->mw->m_dist, (size_t)nq * 8);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// column words -> the mutual flag of every query and (a(j), its distance) of every train descriptor
__global__ void k_mutual_decode(const int32_t* __restrict__ idx, int nq, const uint32_t* __restrict__ colmin, const uint8_t* __restrict__ t, int nt,
                                uint8_t* __restrict__ mutual, int32_t* __restrict__ t_best)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) mutual[i] = knn_mutual(idx[2 * i], i, colmin, nt) ? 1 : 0;
    if (i < nt) {
        const uint32_t key = colmin[i];
        const uint4* tp = (const uint4*)(t + (size_t)i * 32);
        const uint4 a = tp[0], b = tp[1];
        const int tn = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
        const bool h = key != 0xFFFFFFFFu;
        t_best[2 * i] = h ? (int32_t)(key & 0xFFFFu) : -1;
        t_best[2 * i + 1] = h ? (int32_t)(key >> 16) - 256 + tn : 0x7FFFFFFF;
    }
}

extern "C" int vo_bf_knn2_hamming_mutual(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, int32_t* dist,
                                         uint8_t* mutual, int32_t* t_best)
{
    if (!ctx || nq < 0 || nt < 0 || (nq && (!q || !idx || !dist || !mutual)) || (nt && !t))
        return vo_fail(ctx, VO_E_ARG, "vo_bf_knn2_hamming_mutual: bad argument");
    if (nq > ctx->kp_cap || nt > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "descriptor count exceeds capacity %d", ctx->kp_cap);
    if (nq > 65535) return vo_fail(ctx, VO_E_CAP, "cross-check: query set of %d descriptors exceeds 65535", nq);
    if (t_best)
        for (int j = 0; j < nt; j++) { t_best[2 * j] = -1; t_best[2 * j + 1] = 0x7FFFFFFF; }
    if (nq == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    StageTimer tm(ctx, VO_T_MATCH);
    int rc = xfer_h2d(ctx, ctx->mq, q, (size_t)nq * 32);
    if (!rc && nt) rc = xfer_h2d(ctx, ctx->mt, t, (size_t)nt * 32);
    if (rc) return rc;
    if ((rc = match_knn2(ctx, ctx->mq, nq, ctx->mt, nt, ctx->mw->m_idx, ctx->mw->m_dist, 1))) return rc;
    // (the decoded words land in match scratch that nothing else of this call uses: st_a holds kp_cap bytes, xy_a kp_cap pairs)
    int32_t* d_tbest = (int32_t*)ctx->mw->xy_a;
    hipLaunchKernelGGL(k_mutual_decode, dim3(div_up(std::max(nq, std::max(nt, 1)), 256)), dim3(256), 0, ctx->stream, ctx->mw->m_idx, nq,
                       match_colmin(ctx->mw->m_dist, ctx->kp_cap), ctx->mt, nt, ctx->mw->st_a, d_tbest);
    VO_CHECK_LAUNCH(ctx);
    rc = xfer_d2h(ctx, idx, ctx->mw->m_idx, (size_t)nq * 8);
    if (!rc) rc = xfer_d2h(ctx, dist, ctx->mw->m_dist, (size_t)nq * 8);
    if (!rc) rc = xfer_d2h(ctx, mutual, ctx->mw->st_a, (size_t)nq);
    if (!rc && t_best && nt) rc = xfer_d2h(ctx, t_best, d_tbest, (size_t)nt * 8);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// kNN-2 inside a window of the keypoint positions on host arrays (the radii are arguments here: the context's window is neither read
// nor changed); with VO_MATCH_CROSSCHECK also mutual / t_best as vo_bf_knn2_hamming_mutual gives them, mutual within the window
extern "C" int vo_bf_knn2_hamming_window(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, const float* xy_q, const float* xy_t, float rx,
                                         float ry, int match_flags, int32_t* idx, int32_t* dist, uint8_t* mutual, int32_t* t_best)
{
    const int cross = match_flags & VO_MATCH_CROSSCHECK;
    if (!ctx || nq < 0 || nt < 0 || (nq && (!q || !xy_q || !idx || !dist || (cross && !mutual))) || (nt && (!t || !xy_t)) ||
        (match_flags & ~(VO_MATCH_CROSSCHECK | VO_MATCH_WINDOW)))
        return vo_fail(ctx, VO_E_ARG, "vo_bf_knn2_hamming_window: bad argument");
    if (!(rx >= 0.f) || !(ry >= 0.f) || rx > 3.4028234e38f || ry > 3.4028234e38f)
        return vo_fail(ctx, VO_E_ARG, "vo_bf_knn2_hamming_window: the radii must be finite and >= 0");
    if (nq > ctx->kp_cap || nt > ctx->kp_cap) return vo_fail(ctx, VO_E_CAP, "descriptor count exceeds capacity %d", ctx->kp_cap);
    if (cross && nq > 65535) return vo_fail(ctx, VO_E_CAP, "cross-check: query set of %d descriptors exceeds 65535", nq);
    if (cross && t_best)
        for (int j = 0; j < nt; j++) { t_best[2 * j] = -1; t_best[2 * j + 1] = 0x7FFFFFFF; }
    if (nq == 0) return VO_OK;
    VO_HIP(ctx, hipSetDevice(ctx->device));
    StageTimer tm(ctx, VO_T_MATCH);
    int rc = xfer_h2d(ctx, ctx->mq, q, (size_t)nq * 32);
    if (!rc) rc = xfer_h2d(ctx, ctx->mw->xy_a, xy_q, (size_t)nq * 8);
    if (!rc && nt) rc = xfer_h2d(ctx, ctx->mt, t, (size_t)nt * 32);
    if (!rc && nt) rc = xfer_h2d(ctx, ctx->mw->xy_b, xy_t, (size_t)nt * 8);
    if (rc) return rc;
    if ((rc = match_knn2(ctx, ctx->mq, nq, ctx->mt, nt, ctx->mw->m_idx, ctx->mw->m_dist, cross, ctx->mw->xy_a, ctx->mw->xy_b, rx, ry))) return rc;
    int32_t* d_tbest = (int32_t*)ctx->mw->pts_a;     // (kp_cap x 12 bytes: the positions occupy xy_a / xy_b here)
    if (cross) {
        hipLaunchKernelGGL(k_mutual_decode, dim3(div_up(std::max(nq, std::max(nt, 1)), 256)), dim3(256), 0, ctx->stream, ctx->mw->m_idx, nq,
                           match_colmin(ctx->mw->m_dist, ctx->kp_cap), ctx->mt, nt, ctx->mw->st_a, d_tbest);
        VO_CHECK_LAUNCH(ctx);
    }
    rc = xfer_d2h(ctx, idx, ctx->mw->m_idx, (size_t)nq * 8);
    if (!rc) rc = xfer_d2h(ctx, dist, ctx->mw->m_dist, (size_t)nq * 8);
    if (!rc && cross) rc = xfer_d2h(ctx, mutual, ctx->mw->st_a, (size_t)nq);
    if (!rc && cross && t_best && nt) rc = xfer_d2h(ctx, t_best, d_tbest, (size_t)nt * 8);
    if (rc) return rc;
    return xfer_flush(ctx);
}

// ---- asynchronous steps: the one mechanism behind vo_pose_pair_begin / _end and vo_mono_pair_begin / _end (vo_ctx::AsyncAlt) ----
static void alt_release(int kind, vo_ctx::AsyncAlt& p)
{
    if (p.stream) (void)hipStreamSynchronize(p.stream);
    match_ws_free(p.mw);
    if (p.result) (void)hipHostFree(p.result);
    if (p.done) (void)hipEventDestroy(p.done);
    if (p.stream && kind == vo_ctx::ALT_MONO) (void)hipStreamDestroy(p.stream);     // (a pose alternate's stream is one of ctx->pose_streams)
    p = vo_ctx::AsyncAlt();
}

static int alt_prepare(vo_ctx* ctx, int kind, int k)
{
    vo_ctx::AsyncAlt& p = ctx->alt(kind, k);
    if (p.ready) return VO_OK;
    const bool pose = kind == vo_ctx::ALT_POSE;
    hipError_t e = hipSuccess;
    if (pose) {
        hipStream_t& shared = ctx->pose_streams[k % ctx->n_pose_streams];
        if (!shared) e = hipStreamCreateWithFlags(&shared, hipStreamNonBlocking);
        p.stream = shared;
    } else
        e = hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p.done, hipEventDisableTiming);
    // (a pose alternate serves vo_pose_pair_begin, vo_pnp_pair_begin and vo_klt_pnp_pair_begin alike: its record holds a PnpRec with its
    // arrays, the tracked positions of a Lucas-Kanade step included)
    const size_t record = pose ? PNP_HDR + pnp_cap(ctx->kp_cap) * PNP_ARR + 64 : MONO_HDR + (size_t)ctx->kp_cap * (1 + 4 + 4 + 8) + 64;
    if (e == hipSuccess) e = hipHostMalloc((void**)&p.result, record, hipHostMallocDefault);
    if (e == hipSuccess) e = match_ws_alloc(ctx, p.mw, pose ? MATCH_WS_POSE : 0);
    if (e != hipSuccess) {
        alt_release(kind, p);                     // a partly built alternate is given back whole
        return vo_fail(ctx, VO_E_HIP, "asynchronous %s step: allocation failed: %s", pose ? "pose" : "monocular", hipGetErrorString(e));
    }
    p.ready = true;
    return VO_OK;
}

void alt_free(vo_ctx* ctx)
{
    for (int kind : { vo_ctx::ALT_POSE, vo_ctx::ALT_MONO })
        for (int k = 0; k < vo_ctx::alt_count(kind); k++) alt_release(kind, ctx->alt(kind, k));
    for (hipStream_t& st : ctx->pose_streams) {
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
}

int alt_open(vo_ctx* ctx, int kind, FrameSlot& a, FrameSlot& b, const char* who, int* k_out)
{
    const int n = vo_ctx::alt_count(kind), next = ctx->alt_next[kind];
    int k = -1;                                   // the first free alternate from the round-robin position on (tickets need not end in order)
    for (int i = 0; i < n && k < 0; i++)
        if (!ctx->alt(kind, (next + i) % n).busy) k = (next + i) % n;
    if (k < 0)
        return vo_fail(ctx, VO_E_STATE, "%s: every asynchronous %sstep is still open (end one first)", who, kind == vo_ctx::ALT_POSE ? "pose " : "");
    // the first step begun builds EVERY alternate (a dozen allocations, a pinned record and an event each: ~1 ms apiece): built one
    // by one as the round-robin first reaches them, the later ones fell into whatever the caller was timing by then (the first two
    // of bench.py's five cold windows read 10 % low)
    for (int i = 0; i < n; i++)
        if (int rc = alt_prepare(ctx, kind, (k + i) % n)) return rc;
    // the step runs on the alternate's own stream: order it behind whatever still produces the two slots (look-ahead engines)
    // and behind the main stream's work on them
    if (int rc = sweep_group_close_for(ctx, a)) return rc;
    if (int rc = sweep_group_close_for(ctx, b)) return rc;
    // a pose alternate runs on one of the shared pose streams: which of them is decided per step (the alternate is free: its
    // previous step has been waited for, so nothing of it is left on the stream it used then)
    if (kind == vo_ctx::ALT_POSE) ctx->alt(kind, k).stream = ctx->pose_streams[k % pose_stream_count(ctx)];
    const hipStream_t st = ctx->alt(kind, k).stream;
    VO_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipError_t e = hipStreamWaitEvent(st, ctx->ev0, 0);
    if (e == hipSuccess && a.pending) e = hipStreamWaitEvent(st, a.ready, 0);
    if (e == hipSuccess && b.pending) e = hipStreamWaitEvent(st, b.ready, 0);
    if (e != hipSuccess) return vo_fail(ctx, VO_E_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(e));
    *k_out = k;
    return VO_OK;
}

int alt_close(vo_ctx* ctx, int kind, int k, FrameSlot& a, FrameSlot& b, int* ticket_out)
{
    vo_ctx::AsyncAlt& p = ctx->alt(kind, k);
    if (hipEventRecord(p.done, p.stream) != hipSuccess) return vo_fail(ctx, VO_E_HIP, "hipEventRecord failed");
    // both slots are read on this alternate's stream until p.done: whoever refills one of them waits for it first
    slot_add_reader(a, p.done);
    slot_add_reader(b, p.done);
    p.busy = true;
    ctx->alt_next[kind] = (k + 1) % vo_ctx::alt_count(kind);
    *ticket_out = k;
    return VO_OK;
}

int alt_ticket(vo_ctx* ctx, int kind, int ticket, bool args_ok, const char* who)
{
    if (!ctx || !args_ok || ticket < 0 || ticket >= vo_ctx::alt_count(kind)) return vo_fail(ctx, VO_E_ARG, "%s: bad argument", who);
    if (!ctx->alt(kind, ticket).busy) return vo_fail(ctx, VO_E_STATE, "%s: ticket %d is not open", who, ticket);
    return VO_OK;
}

int alt_wait(vo_ctx* ctx, vo_ctx::AsyncAlt& p)
{
    VO_HIP(ctx, hipSetDevice(ctx->device));
    p.busy = false;
    VO_HIP(ctx, hipEventSynchronize(p.done));
    return VO_OK;
}
