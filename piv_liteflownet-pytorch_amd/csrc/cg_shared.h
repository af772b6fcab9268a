// What the conjugate-gradient solvers of pressure.hip and smooth.hip share, and the only place that holds it: the fixed-order sum T(.)
// over the nodes of a frame (include/pivlfn.h, "pressure"), the plan of its block partials, the walk of a workgroup over its tile of
// nodes, the 64-byte record of a system with the heads of the kernels that read it, and the carving of a workspace.
//
// The tree over the N leaves of a frame: a thread owns four consecutive leaves (levels 0, 1), the six levels above cross the lanes of a
// wave (partner lane ^ 1 .. ^ 32; an addition commutes, so both lanes hold the node), two more cross the four waves in LDS: a chunk of
// 1024 leaves.  A workgroup walks `chunks` consecutive chunks (1 up to 2^21 nodes, a power of two beyond) and combines their roots with
// a binary counter, which is the tree's order again, into ONE partial; a frame has at most 2048 partials, and each workgroup of the next
// launch finishes the tree over them in LDS by itself.  Padding is +0.0 and x + (+0.0) = x for every x but -0.0; the leaves r*z and r*r
// of pressure.hip are never negative zero, and of sigma = T(d*q) only `sigma > 0` and rho/sigma for such a sigma are used, so levels
// that add padding above a root change no bit of any result.
//
// A solver's kernel hands pr_tile_roots a leaf callback: leaf(i, l) does node i's loads and stores and fills its K leaves l[0..K-1].
// It is called once for every node of the workgroup's tile, in ascending order, by the thread that owns the node; it may read any node
// of buffers no workgroup of the launch writes and must write node i alone.  It must not synchronise, and it does not see the padding,
// the order of the leaf sums, the chunk roots or the counters: those are the helper's.
#pragma once
#include "common.h"

namespace pivlfn {

constexpr int PR_THREADS = 256, PR_OWN = 4, PR_CHUNK = PR_THREADS * PR_OWN, PR_MAX_PART = 2048;

// ---- the partials plan: chunks per workgroup, partials per frame of N >= 1 nodes ---------------------------------------------------------
struct PrPlan { int chunks, NB; };

static inline PrPlan pr_plan(size_t N)
{
    size_t P2 = 1;
    while (P2 < N) P2 <<= 1;
    const size_t chunks = P2 > (size_t)PR_CHUNK * PR_MAX_PART ? P2 / ((size_t)PR_CHUNK * PR_MAX_PART) : 1;
    const size_t tile = chunks * PR_CHUNK, NB = (N + tile - 1) / tile;
    return {(int)chunks, (int)NB};
}

// Consecutive pieces of a workspace, each rounded up to 8 bytes.  A null base gives the sizes and offsets alone.
struct WsCarver {
    unsigned char *base;
    size_t at = 0;                             // the offset of the next piece; at the end, the bytes of the workspace
    template <typename T>
    T *take(size_t count)
    {
        const size_t o = at;
        at += (sizeof(T) * count + 7) & ~(size_t)7;
        return reinterpret_cast<T *>(base + o);
    }
};

// ---- the tree ---------------------------------------------------------------------------------------------------------------------------
// v[k]: the sum of a thread's four leaves, as (l0 + l1) + (l2 + l3).  Afterwards every thread holds the root of the workgroup's 1024
// leaves.  Called by whole workgroups; sw is [K][4].
template <int K>
__device__ __forceinline__ void pr_chunk_root(double (&v)[K], double (*sw)[4])
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = v[k] + __shfl_xor(v[k], m);
    __syncthreads();                                                           // the last chunk's sums have been read
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sw[k][wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (sw[k][0] + sw[k][1]) + (sw[k][2] + sw[k][3]);
}

// The binary counter over the chunks of a workgroup: up[k] waits for its right sibling at level k above a chunk's root.
// Written without a break so that every index is static and the counter stays in registers.
struct PrCounter {
    double up[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __device__ __forceinline__ double add(double root, int c)
    {
#pragma clang fp contract(off)
        bool carry = true;                                                     // still climbing: every lower bit of c was set
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const bool bit = (c >> k) & 1;
            const double sum = up[k] + root;
            up[k] = (carry && !bit) ? root : up[k];
            root = (carry && bit) ? sum : root;
            carry = carry && bit;
        }
        return root;                                                           // after the last of 2^n chunks: their root
    }
};

// One counter for each of the first K trees of pr_tile_roots: root[k] = the counter of tree k after v[k].  A recursion and not a loop
// over the trees: the level conditions of add do not depend on the tree, the compiler moves them in front of such a loop, and
// smooth_rz_kernel then takes 66 registers for what takes 50.
template <int K>
struct PrCounters : PrCounters<K - 1> {
    PrCounter last;
    template <int N>
    __device__ __forceinline__ void add(const double (&v)[N], double (&root)[N], int c)
    {
        PrCounters<K - 1>::add(v, root, c);
        root[K - 1] = last.add(v[K - 1], c);
    }
};
template <>
struct PrCounters<0> {
    template <int N>
    __device__ __forceinline__ void add(const double (&)[N], double (&)[N], int) {}
};

// The roots of the trees over a frame's NB <= 2048 partials, K trees at once, in every thread: the partials are the leaves of one or two
// chunks, reduced like the nodes' (the padding above a root of fewer than 1024 partials adds +0.0, which changes no result -- see the
// head of the file).  sw is [K][4].
template <int K>
__device__ __forceinline__ void pr_finish(const double *const (&part)[K], int NB, double (*sw)[4], double (&out)[K])
{
#pragma clang fp contract(off)
    for (int c = 0; c * PR_CHUNK < NB; ++c) {
        const int base = c * PR_CHUNK + (int)threadIdx.x * PR_OWN;
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double l[PR_OWN];
#pragma unroll
            for (int j = 0; j < PR_OWN; ++j) l[j] = base + j < NB ? part[k][base + j] : 0.0;
            v[k] = (l[0] + l[1]) + (l[2] + l[3]);
        }
        pr_chunk_root<K>(v, sw);
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = c ? out[k] + v[k] : v[k];
    }
}

// ---- the walk of workgroup blk over its tile: `chunks` chunks of the frame's N nodes, four consecutive nodes a thread ------------------
// fn(i) for every node i < N of the tile, by the thread that owns it
template <typename Fn>
__device__ __forceinline__ void pr_tile_for_each(int chunks, unsigned N, unsigned blk, Fn fn)
{
    for (int c = 0; c < chunks; ++c) {
        const size_t base = ((size_t)blk * chunks + c) * PR_CHUNK + (size_t)threadIdx.x * PR_OWN;
#pragma unroll
        for (int j = 0; j < PR_OWN; ++j)
            if (base + j < N) fn(base + j);
    }
}

// The same walk with K sums over the tile: leaf(i, l) fills the K leaves of node i (see the head of the file), a node past N is K
// leaves of +0.0, and root[k] is the workgroup's partial of tree k in every thread.  Called by whole workgroups with chunks >= 1, which
// pr_plan gives; sw is [K][4].  The index arrives as size_t: a callback that only addresses with it takes it so, one that divides it
// declares it unsigned (N < 2^31).
template <int K, typename Leaf>
__device__ __forceinline__ void pr_tile_roots(int chunks, unsigned N, unsigned blk, double (*sw)[4], double (&root)[K], Leaf leaf)
{
#pragma clang fp contract(off)
    PrCounters<K> cnt;
    for (int c = 0; c < chunks; ++c) {
        const size_t base = ((size_t)blk * chunks + c) * PR_CHUNK + (size_t)threadIdx.x * PR_OWN;
        double l[K][PR_OWN];
#pragma unroll
        for (int j = 0; j < PR_OWN; ++j) {
            double node[K];
#pragma unroll
            for (int k = 0; k < K; ++k) node[k] = 0.0;
            if (base + j < N) leaf(base + j, node);
#pragma unroll
            for (int k = 0; k < K; ++k) l[k][j] = node[k];
        }
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = (l[k][0] + l[k][1]) + (l[k][2] + l[k][3]);
        pr_chunk_root<K>(v, sw);
        cnt.add(v, root, c);
    }
}

// ---- the record of a system (a frame of pressure.hip, a component of a frame of smooth.hip) ----------------------------------------------
static_assert(PIVLFN_PRESSURE_RUNNING == PIVLFN_SMOOTH_RUNNING && PIVLFN_PRESSURE_CONVERGED == PIVLFN_SMOOTH_CONVERGED &&
                  PIVLFN_PRESSURE_BREAKDOWN == PIVLFN_SMOOTH_BREAKDOWN,
              "the shared heads test the states of either solver");

constexpr int CG_FRESH = 0, CG_PENDING = 1, CG_MID = 2;    // what the record and the partials hold: setup's, a half-finished step 5, d*q

struct CgRec {                                 // 64 bytes per system
    double rho, rr, bb;
    int state, iters, phase, dsel;             // dsel: which of the two d buffers holds the current direction
    double unused[3];
};
static_assert(sizeof(CgRec) == 64, "the workspace offsets of include/pivlfn.h count 64 bytes a record");

// field by field, so that a record lives in registers and not in a scratch copy
__device__ __forceinline__ CgRec cg_load(const CgRec *src)
{
    CgRec r;
    r.rho = src->rho, r.rr = src->rr, r.bb = src->bb;
    r.state = src->state, r.iters = src->iters, r.phase = src->phase, r.dsel = src->dsel;
    r.unused[0] = r.unused[1] = r.unused[2] = 0.0;
    return r;
}

__device__ __forceinline__ void cg_store(CgRec *dst, const CgRec &r)
{
    dst->rho = r.rho, dst->rr = r.rr, dst->bb = r.bb;
    dst->state = r.state, dst->iters = r.iters, dst->phase = r.phase, dst->dsel = r.dsel;
}

// ---- the heads the iteration and read-out kernels of both solvers share -------------------------------------------------------------------
// A system that has stopped: its record passes through to the other copy (`writer`: the one thread that writes it) and nothing else
// moves.  true: the workgroup is done.
__device__ __forceinline__ bool cg_frozen(const CgRec &in, CgRec *dst, bool writer)
{
    if (in.state == PIVLFN_PRESSURE_RUNNING) return false;
    if (writer) cg_store(dst, in);
    return true;
}

// The head of an x / r update: sigma = T(d*q) from the partials pdq, the breakdown rule, alpha = rho / sigma.  false: the system broke
// down, its record is written and the workgroup is done.  Called by whole workgroups; sw is [1][4] or larger.
__device__ __forceinline__ bool cg_alpha(const CgRec &in, CgRec *dst, bool writer, const double *pdq, int NB, double (*sw)[4], double &alpha)
{
#pragma clang fp contract(off)
    const double *const parts[1] = {pdq};
    double top[1];
    pr_finish<1>(parts, NB, sw, top);
    const double sigma = top[0];
    if (!(sigma > 0.0)) {                                                      // NaN included
        CgRec out = in;
        out.state = PIVLFN_PRESSURE_BREAKDOWN;
        if (writer) cg_store(dst, out);
        return false;
    }
    alpha = in.rho / sigma;
    return true;
}

// the four doubles of a system's status, by one thread
__device__ __forceinline__ void cg_write_status(double *status, const CgRec &rec)
{
    status[0] = (double)rec.state;
    status[1] = (double)rec.iters;
    status[2] = rec.rr;
    status[3] = rec.bb;
}

}  // namespace pivlfn
