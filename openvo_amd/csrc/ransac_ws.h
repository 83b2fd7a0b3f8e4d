// The device workspaces of the RANSAC steps (ransac.hip), each laid out ONCE: a layout function names its sub-buffers in order,
// runs with a null base to measure the bytes the step needs and with the workspace to hand out the pointers.  Plain host C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

// doubles per hypothesis of the record k_ransac_hyp5 hands to k_ransac_roots5 (fivept.inc describes it)
#define FP_REC_DOUBLES 97

// bump carver: `count` objects of T at the next offset that meets `align` (a power of two; the base is a hipMalloc pointer,
// aligned to 256 bytes at least).  base == NULL: nothing is handed out, `off` ends as the size of the layout.
struct WsCarve {
    uint8_t* base;
    size_t off;
    template <class T> T* take(size_t count, size_t align = alignof(T))
    {
        off = (off + align - 1) & ~(align - 1);
        T* const p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// vo_ransac_essential(5): the models E / F of every hypothesis, the five-point records, the uploaded points, counts, winner, mask
struct EssWs { double *E, *rec; float *p1, *p2, *F; int32_t *counts, *best; uint8_t* mask; };
static inline size_t ess_ws_layout(uint8_t* base, int n, int iters, EssWs* w)
{
    WsCarve c{ base, 0 };
    w->E = c.take<double>((size_t)iters * 9);
    w->rec = c.take<double>((size_t)iters * FP_REC_DOUBLES);
    w->p1 = c.take<float>((size_t)n * 2);
    w->p2 = c.take<float>((size_t)n * 2);
    w->F = c.take<float>((size_t)iters * 9);
    w->counts = c.take<int32_t>((size_t)iters);
    w->best = c.take<int32_t>(64);
    w->mask = c.take<uint8_t>((size_t)n);
    return c.off;
}

// the monocular pair step (the points are the match scratch's xy_a / xy_b); scratch: `extra` bytes for a tail that needs them
struct MonoWs { double *E, *rec; float* F; int32_t *counts, *best; double* E9; uint8_t *mask, *scratch; };
static inline size_t mono_ws_layout(uint8_t* base, int nq, int iters, size_t extra, MonoWs* w)
{
    WsCarve c{ base, 0 };
    w->E = c.take<double>((size_t)iters * 9);
    w->rec = c.take<double>((size_t)iters * FP_REC_DOUBLES);
    w->F = c.take<float>((size_t)iters * 9);
    w->counts = c.take<int32_t>((size_t)iters);
    w->best = c.take<int32_t>(64);
    w->E9 = c.take<double>(32);
    w->mask = c.take<uint8_t>((size_t)nq);
    w->scratch = extra ? c.take<uint8_t>(extra, 256) : nullptr;
    return c.off;
}

// scratch of one pose-recovery tail (rp_tail) over n correspondences and nb keypoints of the second frame
struct RpScratch {
    double *z1, *z2;                      // n each: the winner's depths of the inliers, 0 elsewhere
    unsigned long long* ratio;            // n: scratch of the select
    int32_t* owner;                       // nb: scratch of the scatter
};
static inline size_t rp_scratch_layout(uint8_t* base, int n, int nb, RpScratch* s)
{
    WsCarve c{ base, 0 };
    s->z1 = c.take<double>((size_t)n);
    s->z2 = c.take<double>((size_t)n);
    s->ratio = c.take<unsigned long long>((size_t)n);
    s->owner = c.take<int32_t>((size_t)nb);
    return c.off;
}

// vo_recover_pose: everything the caller uploads, depth_b, then the tail's scratch
struct RecoverWs { double* E; float *p1, *p2; int32_t *q, *t; double *da, *db; uint8_t *mask, *scratch; };
static inline size_t recover_ws_layout(uint8_t* base, int n, int na, int nb, RecoverWs* w)
{
    RpScratch s;
    WsCarve c{ base, 0 };
    w->E = c.take<double>(32);
    w->p1 = c.take<float>((size_t)n * 2);
    w->p2 = c.take<float>((size_t)n * 2);
    w->q = c.take<int32_t>((size_t)n);
    w->t = c.take<int32_t>((size_t)n);
    w->da = c.take<double>((size_t)na, 256);
    w->db = c.take<double>((size_t)nb);
    w->mask = c.take<uint8_t>((size_t)n);
    w->scratch = c.take<uint8_t>(rp_scratch_layout(nullptr, n, nb, &s), 256);
    return c.off;
}

// vo_ransac_pnp: the poses Rt / projections P of every hypothesis, the uploaded points, counts, winner, mask
struct PnpHostWs { double* Rt; float *uv, *X, *P; int32_t *counts, *best; uint8_t* mask; };
static inline size_t pnp_host_ws_layout(uint8_t* base, int n, int iters, PnpHostWs* w)
{
    WsCarve c{ base, 0 };
    w->Rt = c.take<double>((size_t)iters * 12);
    w->uv = c.take<float>((size_t)n * 2);
    w->X = c.take<float>((size_t)n * 3 + 2);
    w->P = c.take<float>((size_t)iters * 12, 16);
    w->counts = c.take<int32_t>((size_t)iters);
    w->best = c.take<int32_t>(64);
    w->mask = c.take<uint8_t>((size_t)n);
    return c.off;
}

// the fused PnP step (pnp_ws_take).  PnpDev: device scratch of one step behind the RANSAC arrays: hdr {M, n, flags}, the n
// usable correspondences in match order
struct PnpDev { int32_t *hdr, *q, *t; float *X, *uv; };
struct PnpWs { double* Rt; float* P; int32_t* counts; PnpDev d; uint8_t* mask; };
static inline size_t pnp_ws_layout(uint8_t* base, int nq, int iters, PnpWs* w)
{
    WsCarve c{ base, 0 };
    w->Rt = c.take<double>((size_t)iters * 12);
    w->P = c.take<float>((size_t)iters * 12);
    w->counts = c.take<int32_t>((size_t)iters);
    w->d.hdr = c.take<int32_t>(64, 256);
    w->d.uv = c.take<float>((size_t)nq * 2);
    w->d.X = c.take<float>((size_t)nq * 3);
    w->d.q = c.take<int32_t>((size_t)nq);
    w->d.t = c.take<int32_t>((size_t)nq);
    w->mask = c.take<uint8_t>((size_t)nq);
    return c.off;
}
