// pointnet2.hip — HomeworkFinal's three classifiers in eval mode: PointNet++ single-scale (SSG; models/pointnet2_cls_ssg.py, models/pointnet_util.py:159-215),
// PointNet++ multi-scale (MSG; models/pointnet2_cls_msg.py) and the vanilla PointNet with its T-Nets (models/pointnet_cls.py, models/pointnet.py).
// The contracts are written out above pcr_pn2_model_create, pcr_pn2_msg_model_create and pcr_pn1_model_create in include/pcr.h.
// Stated once for the three: the layers of a descriptor (pointnet_layers.hpp, the training passes read it too), model_upload, the frame of a forward pass (pass_*).
//
//   pn2_chain_kernel   one workgroup (4 waves) per tile of R = 16 / 32 / 64 ROWS (a row = one sample of one group): gathers the rows' input
//                      channels into LDS, runs the up to four layers relu(W'x + b') with the activations ping-ponging between two LDS
//                      buffers, and reduces the last layer's outputs by group with an atomic max on the bits of the (non-negative) floats.
//                      Products run on v_mfma_f32_16x16x4_f32: A = 16 rows x 4 channels of the activations (one ds_read_b128 per four K
//                      steps), B = 4 channels x 16 outputs of W' (one global_load_dwordx4 per four K steps: the model stores W' in that
//                      operand order), C starts as the bias.  A wave owns output tiles t = wave, wave + 4, ... and all R rows of each, so
//                      every output is ONE chain over ascending k whatever R is, and the max is order-free: the result is the same bits
//                      under every geometry.  The same kernel serves the head (one row per object, no max, no ReLU on the last layer).
//   LDS               a row of a buffer holds Kpad + 4 floats (the + 4 spreads the 16 rows of an operand read over the banks); inside
//                      every block of 16 channels the position 4 q + s holds channel 4 s + q, so that the float4 a lane reads is its
//                      operand of four consecutive K steps.  buffer 0 is as wide as the widest input of an even layer, buffer 1 of an odd one.
//   forward           upload -> per sampling layer { FPS, centres, ball query, memset, chain } -> group_all chain -> head chain -> log_softmax.
//   MSG               (models/pointnet2_cls_msg.py) a layer has up to four branches over one set of centres: one multi-radius ball query, one
//                      scan of the counts (pn2_compact), one memset of the concatenated rows, one chain per branch into its own columns
//                      (out_stride / out_col).  xyz_last puts the features before xyz - centre in layer 0's gather.  With row_ptr a tile row
//                      maps to (group, member) through the scan of the counts: only real hits are run, the copies that pad a row are not.
//   vanilla PointNet  pn1_chain_kernel and its forward pass: described above the kernel.
#include "pcr_internal.hpp"
#include "f32_key.hpp"
#include "pointnet_layers.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int PN2_BLOCK = 256;
constexpr int PN2_WAVES = PN2_BLOCK / 64;
constexpr size_t PN2_LDS_LIMIT = 160 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LayerDev {
    const float* w;      // operand order: [Npad / 16][Kpad / 16][64 lanes][4]: W'[16 t + (lane & 15)][16 kb + 4 s + (lane >> 4)]
    const float* b;      // Npad floats (0 beyond N)
    uint32_t K, Kpad, N, Npad;
};

enum { PN2_GROUPED = 0, PN2_GROUP_ALL = 1, PN2_HEAD = 2 };

struct ChainArgs {
    const float *x, *y, *z;           // the cloud (GROUPED, GROUP_ALL)
    const float *qx, *qy, *qz;        // the centres (GROUPED)
    const uint32_t* seg_ptr;          // n_seg + 1 offsets into the cloud (GROUPED, GROUP_ALL)
    const uint32_t* centre_seg;       // the segment of every centre (GROUPED)
    const uint32_t* idx;              // rows segment-local members (GROUPED)
    const float* feat;                // D floats per point of the cloud; HEAD: per row
    const uint32_t* row_ptr;          // compacted rows (GROUPED): n_groups + 1 offsets, the exclusive scan of the groups' counts; NULL: padded rows
    float* out;                       // groups x out_stride; the chain writes the N columns from out_col on
    uint32_t rows;                    // GROUPED: centres x nsample, GROUP_ALL: points of the segments, HEAD: objects
    uint32_t D, nsample, n_seg, mode, n_layers, s0, s1, p0;
    uint32_t out_stride, out_col, xyz_last, n_groups;
    LayerDev L[PCR_PN2_MAX_MLP];
};

__device__ __forceinline__ float pn2_relu(float v) { return v > 0.0f ? v : 0.0f; }

__device__ __forceinline__ void pn2_atomic_max(float* out, int grp, uint32_t stride, uint32_t c, float m)
{
    if (m > 0.0f) atomicMax((unsigned int*)(out + (size_t)grp * stride + c), __float_as_uint(m));      // out starts at +0; m >= +0: the bits order as the values
}

template <int RT>
__global__ __launch_bounds__(PN2_BLOCK) void pn2_chain_kernel(const ChainArgs a)
{
    constexpr int R = RT * 16;
    extern __shared__ __align__(16) float pn2_lds[];
    float* buf0 = pn2_lds;
    float* buf1 = buf0 + (size_t)R * a.s0;
    uint32_t* rowP = (uint32_t*)(buf1 + (size_t)R * a.s1);      // the point (HEAD: the row) a tile row reads
    int* rowG = (int*)(rowP + R);                               // its group = row of the output, -1: no such row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- the rows of this tile
    uint32_t rows = a.rows;
    if (a.row_ptr) {                                            // compacted: the launch is sized for the padded rows, a tile past the total has nothing to do
        rows = a.row_ptr[a.n_groups];
        if ((unsigned long long)blockIdx.x * R >= rows) return; // block-uniform
    }
    float* const outp = a.out + a.out_col;
    if (tid < R) {
        const unsigned long long g = (unsigned long long)blockIdx.x * R + (unsigned)tid;
        int grp = -1;
        uint32_t p = 0;
        if (g < rows) {
            if (a.mode == PN2_HEAD) {
                p = (uint32_t)g;
                grp = (int)g;
            }
            if (a.mode == PN2_GROUP_ALL) {
                p = a.p0 + (uint32_t)g;
                uint32_t lo = 0, hi = a.n_seg;                  // the last segment that starts at or before p (an empty one never holds p)
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (a.seg_ptr[mid] <= p) lo = mid; else hi = mid;
                }
                grp = (int)lo;
            }
            if (a.mode == PN2_GROUPED) {
                uint32_t q, k;                                  // the group and the member of it
                if (a.row_ptr) {
                    uint32_t lo = 0, hi = a.n_groups;           // the last group that starts at or before g (a group without a hit never holds g)
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (a.row_ptr[mid] <= (uint32_t)g) lo = mid; else hi = mid;
                    }
                    q = lo;
                    k = (uint32_t)g - a.row_ptr[lo];
                } else {
                    q = (uint32_t)(g / a.nsample);
                    k = (uint32_t)(g - (unsigned long long)q * a.nsample);
                }
                const uint32_t s = a.centre_seg[q], base = a.seg_ptr[s], n = a.seg_ptr[s + 1] - base;
                const uint32_t i = k < a.nsample ? a.idx[(size_t)q * a.nsample + k] : n;
                if (i < n) {
                    p = base + i;
                    grp = (int)q;
                } else {
                    grp = -2 - (int)q;                          // a group without a hit (its row holds the segment's size): it leaves its zeros.  Negative
                }                                               // and its own value, so that the rows of a tile still fall into runs of equal groups
            }
        }
        rowP[tid] = p;
        rowG[tid] = grp;
    }
    __syncthreads();
    // ---- layer 0's input: (xyz - centre | features | zeros up to Kpad), or (features | xyz - centre | zeros) with xyz_last; a row without a group is all zeros
    {
        const uint32_t Kp = a.L[0].Kpad;
        for (uint32_t e = (uint32_t)tid; e < (uint32_t)R * Kp; e += PN2_BLOCK) {
            const uint32_t r = e / Kp, pos = e - r * Kp, w = pos & 15u;
            const uint32_t ch = (pos & ~15u) + 4u * (w & 3u) + (w >> 2);
            const int grp = rowG[r];
            const uint32_t p = rowP[r];
            float v = 0.0f;
            if (grp >= 0) {
                if (a.mode == PN2_HEAD) {
                    if (ch < a.D) v = a.feat[(size_t)p * a.D + ch];
                } else if (ch < 3u + a.D) {
                    const uint32_t x0 = a.xyz_last ? a.D : 0u, f0 = a.xyz_last ? 0u : 3u;      // where xyz and the features start
                    if (ch >= x0 && ch < x0 + 3u) {
                        const uint32_t c3 = ch - x0;
                        const float* pc = c3 == 0 ? a.x : (c3 == 1 ? a.y : a.z);
                        v = pc[p];
                        if (a.mode == PN2_GROUPED) {
                            const float* cc = c3 == 0 ? a.qx : (c3 == 1 ? a.qy : a.qz);
                            v = v - cc[grp];
                        }
                    } else {
                        v = a.feat[(size_t)p * a.D + (ch - f0)];
                    }
                }
            }
            buf0[(size_t)r * a.s0 + pos] = v;
        }
    }
    __syncthreads();
    // ---- the layers
    const int j = lane & 15, h = lane >> 4;
    for (uint32_t l = 0; l < a.n_layers; l++) {
        const LayerDev L = a.L[l];
        const float* in = (l & 1u) ? buf1 : buf0;
        float* outb = (l & 1u) ? buf0 : buf1;
        const uint32_t sin = (l & 1u) ? a.s1 : a.s0, sout = (l & 1u) ? a.s0 : a.s1;
        const bool last = l + 1 == a.n_layers;
        const uint32_t KB = L.Kpad >> 4, NT = L.Npad >> 4;
        for (uint32_t t = (uint32_t)wave; t < NT; t += PN2_WAVES) {      // wave-uniform
            const float bias = L.b[t * 16 + j];
            f32x4 acc[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = f32x4{ bias, bias, bias, bias };
            const f32x4* wp = (const f32x4*)L.w + (size_t)t * KB * 64 + lane;
            const float* ap = in + (size_t)j * sin + 4 * h;
            f32x4 bnext = wp[0];
            for (uint32_t kb = 0; kb < KB; kb++) {
                const f32x4 b = bnext;
                if (kb + 1 < KB) bnext = wp[(size_t)(kb + 1) * 64];      // the next block's operand is in flight during this block's products
                f32x4 av[RT];
#pragma unroll
                for (int rt = 0; rt < RT; rt++) av[rt] = *(const f32x4*)(ap + (size_t)rt * 16 * sin + kb * 16);
#pragma unroll
                for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].x, b.x, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].y, b.y, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].z, b.z, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].w, b.w, acc[rt], 0, 0, 0);
            }
            // lane (j, h) holds output channel 16 t + j of the rows 16 rt + 4 h + reg
            if (!last) {
                const uint32_t pos = t * 16 + 4u * (uint32_t)(j & 3) + (uint32_t)(j >> 2);
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) outb[(size_t)(rt * 16 + 4 * h + reg) * sout + pos] = pn2_relu(acc[rt][reg]);
            } else {
                const uint32_t c = t * 16 + (uint32_t)j;
                const bool cvalid = c < L.N;
                if (a.mode == PN2_HEAD) {
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
#pragma unroll
                        for (int reg = 0; reg < 4; reg++) {
                            const int grp = rowG[rt * 16 + 4 * h + reg];
                            if (grp >= 0 && cvalid) outp[(size_t)grp * a.out_stride + c] = acc[rt][reg];
                        }
                } else {
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        const int r0 = rt * 16;
                        const int g0 = rowG[r0], g7 = rowG[r0 + 7], g8 = rowG[r0 + 8], g15 = rowG[r0 + 15];      // the rows of a group are consecutive, -1 only at the tail
                        const float v0 = pn2_relu(acc[rt][0]), v1 = pn2_relu(acc[rt][1]), v2 = pn2_relu(acc[rt][2]), v3 = pn2_relu(acc[rt][3]);
                        if (g0 == g15 || (g0 == g7 && g8 == g15)) {        // wave-uniform: the 16 rows are one group, or two halves of one group each
                            float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
                            m = fmaxf(m, __shfl_xor(m, 16, 64));
                            if (g0 == g15) {
                                m = fmaxf(m, __shfl_xor(m, 32, 64));
                                if (h == 0 && g0 >= 0 && cvalid) pn2_atomic_max(outp, g0, a.out_stride, c, m);
                            } else {
                                const int grp = h < 2 ? g0 : g8;
                                if ((h & 1) == 0 && grp >= 0 && cvalid) pn2_atomic_max(outp, grp, a.out_stride, c, m);
                            }
                        } else {                                            // runs of equal groups inside the lane's four rows
                            const float v[4] = { v0, v1, v2, v3 };
                            int cur = rowG[r0 + 4 * h];
                            float m = v[0];
#pragma unroll
                            for (int reg = 1; reg < 4; reg++) {
                                const int grp = rowG[r0 + 4 * h + reg];
                                if (grp != cur) {
                                    if (cur >= 0 && cvalid) pn2_atomic_max(outp, cur, a.out_stride, c, m);
                                    cur = grp;
                                    m = v[reg];
                                } else {
                                    m = fmaxf(m, v[reg]);
                                }
                            }
                            if (cur >= 0 && cvalid) pn2_atomic_max(outp, cur, a.out_stride, c, m);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// centres of a sampling layer: the picked points of every object (objects of n points, npoint picks each)
__global__ __launch_bounds__(PN2_BLOCK) void pn2_centres_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                                const uint32_t* __restrict__ fps, uint32_t n, uint32_t npoint, uint32_t total,
                                                                float* __restrict__ cx, float* __restrict__ cy, float* __restrict__ cz)
{
    const uint32_t q = blockIdx.x * PN2_BLOCK + threadIdx.x;
    if (q >= total) return;
    uint32_t i = fps[q];
    if (i >= n) i = n - 1;      // (never: a pick is a member)
    const size_t p = (size_t)(q / npoint) * n + i;
    cx[q] = x[p]; cy[q] = y[p]; cz[q] = z[p];
}

// log_softmax of a row of logits and its first maximum: one lane per object, ascending class order
__global__ __launch_bounds__(PN2_BLOCK) void pn2_logsoftmax_kernel(const float* __restrict__ logits, uint32_t n_obj, uint32_t n_class, float* __restrict__ logp,
                                                                   int32_t* __restrict__ pred)
{
    const uint32_t o = blockIdx.x * PN2_BLOCK + threadIdx.x;
    if (o >= n_obj) return;
    const float* r = logits + (size_t)o * n_class;
    float m = r[0];
    int32_t best = 0;
    for (uint32_t c = 1; c < n_class; c++)
        if (r[c] > m) { m = r[c]; best = (int32_t)c; }
    float s = 0.0f;
    for (uint32_t c = 0; c < n_class; c++) s = s + expf(r[c] - m);
    const float ls = logf(s);
    for (uint32_t c = 0; c < n_class; c++) logp[(size_t)o * n_class + c] = (r[c] - m) - ls;
    pred[o] = best;
}

inline uint32_t pad16(uint32_t v) { return (v + 15u) & ~15u; }

// a chain of layers as the kernel takes it
struct Chain {
    uint32_t n = 0;
    LayerDev L[PCR_PN2_MAX_MLP];
    uint32_t s0 = 4, s1 = 4;
    uint32_t n_out() const { return L[n - 1].N; }
    size_t lds_bytes(int R) const { return (size_t)R * (s0 + s1) * 4 + (size_t)R * 8; }
};

// rows per tile: the tuned value if it fits, else the largest of 64 / 32 / 16 that does (16 always does: two rows of 1028 floats x 16 = 129 KB)
template <class C>
int chain_rows(const pcr_ctx* ctx, const C& ch)
{
    const int64_t want = tune_get(ctx, "pn2_rows", 0);
    const int cand[3] = { 64, 32, 16 };
    for (int k = 0; k < 3; k++)
        if ((want == 0 || cand[k] <= want) && ch.lds_bytes(cand[k]) <= PN2_LDS_LIMIT) return cand[k];
    return 16;
}

// the two LDS row strides of a chain (Chain) or a stage (Pn1Stage): buffer 0 holds the inputs of the even layers, buffer 1 of the odd ones
template <class C>
void lds_strides(C& ch)
{
    ch.s0 = ch.s1 = 4;
    for (uint32_t l = 0; l < ch.n; l++) {
        uint32_t& s = (l & 1u) ? ch.s1 : ch.s0;
        s = std::max(s, ch.L[l].Kpad + 4);
    }
}

// one instance of a chain kernel (pn2_chain_kernel<RT> / pn1_chain_kernel<RT>) with its dynamic LDS
template <auto Kernel, class A>
int launch_rt(pcr_ctx* ctx, const A& a, size_t lds, unsigned blocks)
{
    PCR_HIP(ctx, hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(PN2_BLOCK), lds, ctx->stream, a);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// columns [a.out_col, a.out_col + n_out) of a.out (n_groups x a.out_stride; 0 = n_out) <- the chain over a.rows rows; enqueued on the stream.
// clear: the rows of a.out are zeroed first, under the same profile scope — the caller of a layer with several branches asks for it ONCE, with
// its first branch (the max is taken with atomics on rows that start at +0).
int chain_launch(pcr_ctx* ctx, const Chain& ch, ChainArgs a, size_t n_groups, const char* prof, bool clear = true)
{
    if (a.rows == 0 || n_groups == 0) return PCR_OK;
    a.n_layers = ch.n;
    a.s0 = ch.s0;
    a.s1 = ch.s1;
    a.n_groups = (uint32_t)n_groups;
    if (a.out_stride == 0) a.out_stride = ch.n_out();
    for (uint32_t l = 0; l < ch.n; l++) a.L[l] = ch.L[l];
    const int R = chain_rows(ctx, ch);
    const size_t lds = ch.lds_bytes(R);
    if (lds > PN2_LDS_LIMIT) return fail(ctx, PCR_ERR_STATE, "pointnet2: a chain does not fit in LDS");
    ProfScope ps(ctx, prof);
    if (a.mode != PN2_HEAD && clear) PCR_HIP(ctx, hipMemsetAsync(a.out, 0, n_groups * a.out_stride * 4, ctx->stream));
    const unsigned tiles = (unsigned)(((unsigned long long)a.rows + R - 1) / R);
    return R == 64 ? launch_rt<pn2_chain_kernel<4>>(ctx, a, lds, tiles) : R == 32 ? launch_rt<pn2_chain_kernel<2>>(ctx, a, lds, tiles) : launch_rt<pn2_chain_kernel<1>>(ctx, a, lds, tiles);
}

// one row per object through FC layers (the classifier's head, a T-Net's): in = n_obj x width, out = n_obj x the chain's last width
int head_launch(pcr_ctx* ctx, const Chain& ch, const float* in, uint32_t width, float* out, size_t n_obj)
{
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.feat = in; a.out = out;
    a.rows = (uint32_t)n_obj;
    a.D = width; a.nsample = 1; a.mode = PN2_HEAD;
    return chain_launch(ctx, ch, a, n_obj, "pn2_head");
}

// row_ptr[b][0 .. nq] <- the exclusive scan of counts[b][0 .. nq), for every branch b = blockIdx.x in ONE launch.  A thread sums a run of
// consecutive counts, the 256 sums are scanned in LDS, the thread writes its run.
__global__ __launch_bounds__(PN2_BLOCK) void pn2_scan_kernel(const uint32_t* __restrict__ counts, uint32_t nq, uint32_t* __restrict__ row_ptr)
{
    __shared__ uint32_t part[PN2_BLOCK];
    const uint32_t* c = counts + (size_t)blockIdx.x * nq;
    uint32_t* rp = row_ptr + (size_t)blockIdx.x * ((size_t)nq + 1);
    const uint32_t per = (nq + PN2_BLOCK - 1) / PN2_BLOCK;
    const unsigned long long lo64 = (unsigned long long)threadIdx.x * per;
    const uint32_t lo = lo64 < nq ? (uint32_t)lo64 : nq, hi = lo64 + per < nq ? (uint32_t)(lo64 + per) : nq;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += c[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < PN2_BLOCK; d <<= 1) {                   // inclusive scan of the 256 sums
        const uint32_t v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; i++) { rp[i] = run; run += c[i]; }
    if (threadIdx.x == PN2_BLOCK - 1) rp[nq] = part[PN2_BLOCK - 1];
}

int scan_launch(pcr_ctx* ctx, const uint32_t* counts_dev, size_t nq, size_t n_branch, uint32_t* row_ptr_dev)
{
    if (nq == 0 || n_branch == 0) return PCR_OK;
    ProfScope ps(ctx, "pn2_scan");
    hipLaunchKernelGGL(pn2_scan_kernel, dim3((unsigned)n_branch), dim3(PN2_BLOCK), 0, ctx->stream, counts_dev, (uint32_t)nq, row_ptr_dev);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// pn2_compact: -1 / unset = the model's default, 0 = padded rows, anything else = compacted
bool compact_rows(const pcr_ctx* ctx, bool model_default)
{
    auto it = ctx->tune.find("pn2_compact");
    if (it == ctx->tune.end() || it->second < 0) return model_default;
    return it->second != 0;
}

bool seg_ok(const uint32_t* seg_ptr, size_t n_seg, size_t limit)
{
    for (size_t s = 0; s < n_seg; s++)
        if (seg_ptr[s] > seg_ptr[s + 1]) return false;
    return seg_ptr[n_seg] <= limit;
}

// ---- the vanilla PointNet (models/pointnet_cls.py, models/pointnet.py): the contract is above pcr_pn1_model_create in include/pcr.h -------------
//   pn1_chain_kernel  one workgroup per tile of R rows = R consecutive points of ONE object (block -> (object, tile of it); an object of fewer
//                     tiles than the launch has per object returns at once), so the object's own matrices serve every row of the tile:
//                     gather (xyz . T3 as three plain fmaf per coordinate | features) -> up to five STEPS ping-ponging between the two LDS
//                     buffers, a step being a convolution of the model (pn2_chain_kernel's products, W' from global memory) or the K x K
//                     transform (the same products with the object's matrix staged in LDS in W's operand order, accumulators starting at +0,
//                     no ReLU) -> the max over the tile's real rows on the integer key of f32_key.hpp, one atomicMax per column and tile.
//   output            rows of keys that start at KEY_NINF; pn1_decode_kernel turns them into floats in place once the chain is done.
constexpr int PN1_MAX_STEPS = 5;             // convolution 0, the transform (K <= PN_MAX_TRANSFORM: the matrix takes Kpad^2 floats of LDS), three more convolutions

struct Pn1Stage {
    uint32_t n = 0;                          // steps; 0: the model has no such stage
    LayerDev L[PN1_MAX_STEPS];               // the transform step: w = b = NULL, K = N = the matrix's size
    uint32_t t_step = UINT32_MAX;            // which step is the transform
    uint32_t relu_last = 1, s0 = 4, s1 = 4;
    uint32_t n_out() const { return L[n - 1].N; }
    size_t lds_bytes(int R) const { return ((size_t)R * (s0 + s1) + (t_step < n ? (size_t)L[t_step].Kpad * L[t_step].Npad : 0)) * 4; }
};

struct Pn1Args {
    const float *x, *y, *z;                  // the cloud
    const float* feat;                       // D floats per point of the cloud
    const uint32_t* seg_ptr;                 // n_seg + 1 offsets into the cloud: a segment is an object
    const float* trans3;                     // n_seg x 9 or NULL
    const float* transK;                     // n_seg x K x K: the matrices of the transform step
    uint32_t* out;                           // n_seg x N keys
    uint32_t D, tiles_per_seg, n_steps, t_step, relu_last, s0, s1;
    LayerDev L[PN1_MAX_STEPS];
};

// acc (starting at the bias) += the K products of one 16-column output tile for the RT row tiles; wp: the tile's operand blocks at this lane.
// (pn2_chain_kernel keeps this loop inline: called from there it kept registers and occupancy, but pn2_sa of the MSG model ran 1.35 % longer; the record is the
// last section of profiles/pointnet2_msg.txt)
template <int RT>
__device__ __forceinline__ void pn1_products(f32x4 (&acc)[RT], const f32x4* wp, const float* ap, uint32_t sin, uint32_t KB)
{
    f32x4 bnext = wp[0];
    for (uint32_t kb = 0; kb < KB; kb++) {
        const f32x4 b = bnext;
        if (kb + 1 < KB) bnext = wp[(size_t)(kb + 1) * 64];
        f32x4 av[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) av[rt] = *(const f32x4*)(ap + (size_t)rt * 16 * sin + kb * 16);
#pragma unroll
        for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].x, b.x, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].y, b.y, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].z, b.z, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; rt++) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].w, b.w, acc[rt], 0, 0, 0);
    }
}

template <int RT>
__global__ __launch_bounds__(PN2_BLOCK) void pn1_chain_kernel(const Pn1Args a)
{
    constexpr int R = RT * 16;
    extern __shared__ __align__(16) float pn1_lds[];
    float* buf0 = pn1_lds;
    float* buf1 = buf0 + (size_t)R * a.s0;
    float* tmat = buf1 + (size_t)R * a.s1;                      // the object's K x K matrix in W's operand order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t seg = blockIdx.x / a.tiles_per_seg, tile = blockIdx.x - seg * a.tiles_per_seg;
    const uint32_t base = a.seg_ptr[seg], n = a.seg_ptr[seg + 1] - base;
    if ((unsigned long long)tile * R >= n) return;              // block-uniform: this object has fewer tiles
    const uint32_t r0 = tile * (uint32_t)R, nrows = n - r0 < (uint32_t)R ? n - r0 : (uint32_t)R;
    // ---- step 0's input: (xyz . T3 | features | zeros up to Kpad); a row past the object's end is all zeros
    {
        const uint32_t Kp = a.L[0].Kpad;
        const float* t3 = a.trans3 ? a.trans3 + (size_t)seg * 9 : nullptr;
        for (uint32_t e = (uint32_t)tid; e < (uint32_t)R * Kp; e += PN2_BLOCK) {
            const uint32_t r = e / Kp, pos = e - r * Kp, w = pos & 15u;
            const uint32_t ch = (pos & ~15u) + 4u * (w & 3u) + (w >> 2);
            float v = 0.0f;
            if (r < nrows && ch < 3u + a.D) {
                const size_t p = (size_t)base + r0 + r;
                if (ch >= 3u) {
                    v = a.feat[p * a.D + (ch - 3u)];
                } else if (t3) {                                // y[ch] = sum_k x[k] T[k][ch]: one chain from +0, k ascending
                    v = fmaf(a.x[p], t3[ch], 0.0f);
                    v = fmaf(a.y[p], t3[3 + ch], v);
                    v = fmaf(a.z[p], t3[6 + ch], v);
                } else {
                    v = (ch == 0 ? a.x : (ch == 1 ? a.y : a.z))[p];
                }
            }
            buf0[(size_t)r * a.s0 + pos] = v;
        }
    }
    if (a.t_step < a.n_steps) {                                 // position ((t KB + kb) 64 + lane) 4 + s holds W'[n][k] = T[k][n], n = 16 t + (lane & 15), k = 16 kb + 4 s + (lane >> 4)
        const uint32_t K = a.L[a.t_step].K, Kp = a.L[a.t_step].Kpad, KB = Kp >> 4;
        const float* T = a.transK + (size_t)seg * K * K;
        for (uint32_t e = (uint32_t)tid; e < Kp * Kp; e += PN2_BLOCK) {
            const uint32_t s = e & 3u, ln = (e >> 2) & 63u, blk = e >> 8, kb = blk % KB, t = blk / KB;
            const uint32_t k = 16u * kb + 4u * s + (ln >> 4), nn = 16u * t + (ln & 15u);
            tmat[e] = (k < K && nn < K) ? T[(size_t)k * K + nn] : 0.0f;
        }
    }
    __syncthreads();
    // ---- the steps
    const int j = lane & 15, h = lane >> 4;
    for (uint32_t l = 0; l < a.n_steps; l++) {
        const LayerDev L = a.L[l];
        const float* in = (l & 1u) ? buf1 : buf0;
        float* outb = (l & 1u) ? buf0 : buf1;
        const uint32_t sin = (l & 1u) ? a.s1 : a.s0, sout = (l & 1u) ? a.s0 : a.s1;
        const bool last = l + 1 == a.n_steps, transform = l == a.t_step;
        const uint32_t KB = L.Kpad >> 4, NT = L.Npad >> 4;
        for (uint32_t t = (uint32_t)wave; t < NT; t += PN2_WAVES) {      // wave-uniform
            const float bias = transform ? 0.0f : L.b[t * 16 + j];
            f32x4 acc[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = f32x4{ bias, bias, bias, bias };
            const float* ap = in + (size_t)j * sin + 4 * h;
            if (transform) pn1_products<RT>(acc, (const f32x4*)tmat + (size_t)t * KB * 64 + lane, ap, sin, KB);
            else pn1_products<RT>(acc, (const f32x4*)L.w + (size_t)t * KB * 64 + lane, ap, sin, KB);
            // lane (j, h) holds output channel 16 t + j of the rows 16 rt + 4 h + reg
            if (!last) {
                const uint32_t pos = t * 16 + 4u * (uint32_t)(j & 3) + (uint32_t)(j >> 2);
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++)
                        outb[(size_t)(rt * 16 + 4 * h + reg) * sout + pos] = transform ? acc[rt][reg] : pn2_relu(acc[rt][reg]);
            } else {
                uint32_t m = 0;                                          // below the key of every float the chain can give
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const float v = a.relu_last ? pn2_relu(acc[rt][reg]) : acc[rt][reg];
                        const uint32_t key = f32_key(v);
                        if ((uint32_t)(rt * 16 + 4 * h + reg) < nrows && key > m) m = key;
                    }
                uint32_t o = __shfl_xor(m, 16, 64);
                m = o > m ? o : m;
                o = __shfl_xor(m, 32, 64);
                m = o > m ? o : m;
                const uint32_t c = t * 16 + (uint32_t)j;
                if (h == 0 && c < L.N) atomicMax(a.out + (size_t)seg * L.N + c, m);      // the tile holds a real row: m is a float's key
            }
        }
        __syncthreads();
    }
}

// t[o] (k x k, row-major) += the identity: ONE f32 addition per diagonal entry, after the T-Net's last chain, as the reference adds it (pointnet.py:41-46)
__global__ __launch_bounds__(PN2_BLOCK) void pn1_identity_kernel(float* __restrict__ t, uint32_t n_obj, uint32_t k)
{
    const size_t i = (size_t)blockIdx.x * PN2_BLOCK + threadIdx.x;
    if (i >= (size_t)n_obj * k) return;
    const size_t o = i / k, d = i - o * k;
    float* p = t + (o * k + d) * k + d;
    *p = *p + 1.0f;
}

__global__ __launch_bounds__(PN2_BLOCK) void pn1_decode_kernel(uint32_t* __restrict__ keys, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PN2_BLOCK + threadIdx.x;
    if (i < n) keys[i] = __float_as_uint(f32_from_key(keys[i]));
}

// a.out (n_seg x n_out floats) <- the stage over the n_seg segments of a.seg_ptr, none longer than max_pts; enqueued on the stream
int pn1_launch(pcr_ctx* ctx, const Pn1Stage& st, Pn1Args a, size_t n_seg, size_t max_pts)
{
    if (n_seg == 0) return PCR_OK;
    a.n_steps = st.n; a.t_step = st.t_step; a.relu_last = st.relu_last; a.s0 = st.s0; a.s1 = st.s1;
    for (uint32_t l = 0; l < st.n; l++) a.L[l] = st.L[l];
    const int R = chain_rows(ctx, st);
    const size_t lds = st.lds_bytes(R), cells = n_seg * st.n_out();
    if (lds > PN2_LDS_LIMIT) return fail(ctx, PCR_ERR_STATE, "pointnet: a stage does not fit in LDS");
    const unsigned long long tiles = (max_pts + R - 1) / R, blocks = tiles * n_seg;
    if (blocks > PN_MAX_ROWS) return fail(ctx, PCR_ERR_ARG, "pointnet: too many tiles (segments x tiles of the longest one)");
    a.tiles_per_seg = (uint32_t)tiles;
    ProfScope ps(ctx, "pn1_chain");
    PCR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)a.out, (int)KEY_NINF, cells, ctx->stream));
    if (blocks) {
        const unsigned nb = (unsigned)blocks;
        const int rc = R == 64 ? launch_rt<pn1_chain_kernel<4>>(ctx, a, lds, nb) : R == 32 ? launch_rt<pn1_chain_kernel<2>>(ctx, a, lds, nb) : launch_rt<pn1_chain_kernel<1>>(ctx, a, lds, nb);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(pn1_decode_kernel, dim3((unsigned)((cells + PN2_BLOCK - 1) / PN2_BLOCK)), dim3(PN2_BLOCK), 0, ctx->stream, a.out, cells);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

}  // namespace

}  // namespace pcr

using namespace pcr;

struct pcr_pn2_model {
    pcr_pn2_msg_desc desc = {};      // every model is held in the superset descriptor
    pcr_pn2_desc ssg = {};           // the single-scale descriptor, where it can express the model (has_ssg)
    bool has_ssg = false;
    bool compact_default = false;    // pn2_compact of a context that does not set it
    int device = 0;
    float* dev = nullptr;            // every layer's operands and biases: the model owns the block
    ~pcr_pn2_model() { if (dev) (void)hipFree(dev); }
    Chain sa[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH];
    Chain head;
    uint32_t sa_in[PCR_PN2_MAX_SA];  // input channels of every SA layer (3 + D)
    uint32_t sa_out[PCR_PN2_MAX_SA]; // its width: the sum of its branches' last widths
    uint64_t n_weights = 0;
    uint32_t n_sampling = 0;
    // ---- a model of pcr_pn1_model_create (the vanilla PointNet): desc / ssg / sa stay empty, head is the classifier's
    bool pn1 = false;
    pcr_pn1_desc d1 = {};
    Pn1Stage stage[3];               // the fused point stages (n == 0: the model has no such stage)
    Chain tnet_head[2];              // the FC layers of the input / the feature T-Net: -> 9 / K x K floats per object, before the identity is added
};

namespace {

// BN folded (f64, rounded once) into the operand order of the kernel: img <- every layer's W' block and bias, w_off / b_off <- where they start.
// NULL, or what is wrong with the weights
const char* fold_layers(const std::vector<LayerShape>& shapes, const float* weights, double bn_eps, std::vector<float>& img, std::vector<size_t>& w_off,
                        std::vector<size_t>& b_off)
{
    size_t dev_floats = 0;
    w_off.resize(shapes.size());
    b_off.resize(shapes.size());
    for (size_t i = 0; i < shapes.size(); i++) {
        const size_t Kp = pad16(shapes[i].K), Np = pad16(shapes[i].N);
        w_off[i] = dev_floats; dev_floats += Kp * Np;
        b_off[i] = dev_floats; dev_floats += Np;
        dev_floats = (dev_floats + 63) & ~(size_t)63;      // every operand block starts on 256 bytes
    }
    img.assign(dev_floats, 0.0f);
    const float* p = weights;
    for (size_t i = 0; i < shapes.size(); i++) {
        const uint32_t K = shapes[i].K, N = shapes[i].N, Kp = pad16(K), KB = Kp / 16;
        const float *W = p, *b = W + (size_t)K * N;
        const float *gamma = b + N, *beta = gamma + N, *mean = beta + N, *var = mean + N;
        p = shapes[i].bn ? var + N : b + N;
        for (uint32_t n = 0; n < N; n++) {
            double s = 1.0, bb = (double)b[n];
            if (shapes[i].bn) {
                const double v = (double)var[n] + bn_eps;
                if (!(v > 0.0)) return ": running_var + eps must be positive";
                s = (double)gamma[n] / std::sqrt(v);
                bb = ((double)b[n] - (double)mean[n]) * s + (double)beta[n];
            }
            const float bf = (float)bb;
            if (!std::isfinite(bf)) return ": a folded bias is not finite";
            img[b_off[i] + n] = bf;
            const uint32_t t = n / 16, j = n % 16;
            for (uint32_t k = 0; k < K; k++) {
                const float wf = (float)(s * (double)W[(size_t)n * K + k]);
                if (!std::isfinite(wf)) return ": a folded weight is not finite";
                const uint32_t kb = k / 16, sidx = (k % 16) / 4, q = k % 4;
                img[w_off[i] + (((size_t)t * KB + kb) * 64 + (q * 16 + j)) * 4 + sidx] = wf;
            }
        }
    }
    return nullptr;
}

// what every create does once the layers are known: the count check, the finite check, the fold, the device block and its upload.  m <- a fresh model that
// owns the block, layer[i] <- layer i as the kernels take it.  who: the entry point, for the argument messages; family: "pointnet2" / "pointnet"
int model_upload(pcr_ctx* ctx, const char* who, const char* family, const std::vector<LayerShape>& shapes, const float* weights, size_t n_weights, double bn_eps,
                 std::unique_ptr<pcr_pn2_model>& m, std::vector<LayerDev>& layer)
{
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str()); };
    const uint64_t need = weight_count(shapes);
    if (n_weights != need) return bad(": n_weights is not the model's count");
    for (size_t i = 0; i < n_weights; i++)
        if (!std::isfinite(weights[i])) return bad(": a non-finite weight");
    std::vector<float> img;
    std::vector<size_t> w_off, b_off;
    if (const char* what = fold_layers(shapes, weights, bn_eps, img, w_off, b_off)) return bad(what);
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    m.reset(new pcr_pn2_model());
    m->device = ctx->device;
    m->n_weights = need;
    PCR_HIP(ctx, hipMalloc((void**)&m->dev, img.size() * 4));
    const hipError_t e = hipMemcpy(m->dev, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, (std::string(family) + ": the upload of a model").c_str(), e);
    for (size_t i = 0; i < shapes.size(); i++)
        layer.push_back({ m->dev + w_off[i], m->dev + b_off[i], shapes[i].K, pad16(shapes[i].K), shapes[i].N, pad16(shapes[i].N) });
    return PCR_OK;
}

// the model of a descriptor; ssg: the single-scale descriptor it was made from, or NULL.  who: the entry point, for the messages
int model_build(pcr_ctx* ctx, const pcr_pn2_msg_desc* desc, const pcr_pn2_desc* ssg, const float* weights, size_t n_weights, pcr_pn2_model** out, const char* who,
                bool compact_default)
{
    Pn2Layers ly;
    if (!pn2_layers(*desc, ly)) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a descriptor outside the limits (see include/pcr.h)").c_str());
    std::unique_ptr<pcr_pn2_model> m;
    std::vector<LayerDev> layer;
    const int rc = model_upload(ctx, who, "pointnet2", ly.shapes, weights, n_weights, desc->bn_eps, m, layer);
    if (rc) return rc;
    m->desc = *desc;
    if (ssg) m->ssg = *ssg;
    m->has_ssg = ssg != nullptr;
    m->compact_default = compact_default;
    m->n_sampling = ly.n_sampling;
    for (uint32_t l = 0; l < desc->n_sa; l++) {
        for (uint32_t b = 0; b < desc->sa[l].n_branch; b++) {
            Chain& ch = m->sa[l][b];
            ch.n = desc->sa[l].branch[b].n_mlp;
            for (uint32_t k = 0; k < ch.n; k++) ch.L[k] = layer[ly.first[l][b] + k];
            lds_strides(ch);
        }
        m->sa_in[l] = ly.sa_in[l];
        m->sa_out[l] = ly.sa_out[l];
    }
    m->head.n = desc->n_fc;
    for (uint32_t k = 0; k < m->head.n; k++) m->head.L[k] = layer[ly.head_first + k];
    lds_strides(m->head);
    *out = m.release();
    return PCR_OK;
}

}  // namespace

extern "C" int pcr_pn2_model_create(pcr_ctx* ctx, const pcr_pn2_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out)
{
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_model_create");
    pcr_pn2_msg_desc d;                      // the same model in the superset descriptor
    if (!pn2_msg_desc_of(*desc, d)) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_model_create: a descriptor outside the limits (see include/pcr.h)");
    return model_build(ctx, &d, desc, weights, n_weights, out, "pcr_pn2_model_create", false);
}

extern "C" int pcr_pn2_msg_model_create(pcr_ctx* ctx, const pcr_pn2_msg_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out)
{
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_msg_model_create");
    pcr_pn2_desc s;                          // the single-scale descriptor, if every layer has one xyz-first branch
    memset(&s, 0, sizeof(s));
    bool single = desc->n_sa >= 1 && desc->n_sa <= PCR_PN2_MAX_SA;
    for (uint32_t l = 0; single && l < desc->n_sa; l++) single = desc->sa[l].n_branch == 1 && desc->sa[l].xyz_last == 0;
    if (single) {
        s.D0 = desc->D0; s.n_sa = desc->n_sa; s.n_fc = desc->n_fc; s.bn_eps = desc->bn_eps;
        for (uint32_t k = 0; k < PCR_PN2_MAX_FC; k++) s.fc_widths[k] = desc->fc_widths[k];
        for (uint32_t l = 0; l < desc->n_sa; l++) {
            const pcr_pn2_msg_sa_desc& m = desc->sa[l];
            s.sa[l].npoint = m.npoint; s.sa[l].group_all = m.group_all;
            s.sa[l].radius = m.branch[0].radius; s.sa[l].nsample = m.branch[0].nsample; s.sa[l].n_mlp = m.branch[0].n_mlp;
            for (uint32_t k = 0; k < PCR_PN2_MAX_MLP; k++) s.sa[l].widths[k] = m.branch[0].widths[k];
        }
    }
    return model_build(ctx, desc, single ? &s : nullptr, weights, n_weights, out, "pcr_pn2_msg_model_create", true);
}

extern "C" int pcr_pn2_model_destroy(pcr_ctx* ctx, pcr_pn2_model* model)
{
    if (!model) return PCR_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete model;                            // frees its device block
    return PCR_OK;
}

namespace {

// the figures of a descriptor (which pn2_layers accepts): they do not need the device
bool desc_info(const pcr_pn2_msg_desc& d, size_t npts_hint, pcr_pn2_info* info)
{
    Pn2Layers ly;
    if (!pn2_layers(d, ly)) return false;
    const std::vector<LayerShape>& shapes = ly.shapes;
    memset(info, 0, sizeof(*info));
    info->n_weights = weight_count(shapes);
    info->n_class = d.fc_widths[d.n_fc - 1];
    info->c_last = ly.sa_out[d.n_sa - 1];
    info->n_sampling = ly.n_sampling;
    uint64_t macs = 0, n = npts_hint;
    size_t i = 0;
    for (uint32_t l = 0; l < d.n_sa; l++) {
        const pcr_pn2_msg_sa_desc& s = d.sa[l];
        for (uint32_t b = 0; b < s.n_branch; b++) {
            uint64_t per_row = 0;
            for (uint32_t k = 0; k < s.branch[b].n_mlp; k++, i++) per_row += (uint64_t)shapes[i].K * shapes[i].N;
            macs += per_row * (s.group_all ? n : (uint64_t)s.npoint * s.branch[b].nsample);
        }
        n = s.group_all ? 1 : s.npoint;
    }
    for (; i < shapes.size(); i++) macs += (uint64_t)shapes[i].K * shapes[i].N;
    info->macs_per_object = macs;
    return true;
}

}  // namespace

extern "C" int pcr_pn2_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn2_desc* desc)
{
    if (!model || model->pn1) return PCR_ERR_ARG;
    if (desc) {
        if (!model->has_ssg) return PCR_ERR_ARG;      // several branches or features-first channels: only pcr_pn2_msg_desc holds them
        *desc = model->ssg;
    }
    if (info) (void)desc_info(model->desc, npts_hint, info);
    return PCR_OK;
}

extern "C" int pcr_pn2_msg_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn2_msg_desc* desc)
{
    if (!model) {                            // no model: *desc is READ, info is what a model made from it would report (no device needed)
        if (!desc || !info) return PCR_ERR_ARG;
        return desc_info(*desc, npts_hint, info) ? PCR_OK : PCR_ERR_ARG;
    }
    if (model->pn1) return PCR_ERR_ARG;      // pcr_pn1_model_info holds its descriptor
    if (desc) *desc = model->desc;
    if (info) (void)desc_info(model->desc, npts_hint, info);
    return PCR_OK;
}

namespace {

// one SA layer on the caller's indices.  msg: pcr_sa_msg_mlp_max_f32 (every branch, idx = the branches' row blocks, an all-N row is a group
// without a hit); else pcr_sa_mlp_max_f32 (one branch, every index inside its segment)
int sa_layer(pcr_ctx* ctx, const pcr_pn2_model* model, int layer, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres,
             const uint32_t* centre_seg_ptr, size_t n_seg, const float* features, const uint32_t* idx, float* out, bool msg)
{
    const std::string who = msg ? "pcr_sa_msg_mlp_max_f32" : "pcr_sa_mlp_max_f32";
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (who + what).c_str()); };
    if (!ctx || !model || !cloud || !seg_ptr) return bad("");
    if (model->pn1) return bad(": a model of pcr_pn1_model_create has no SA layers");
    if (layer < 0 || (uint32_t)layer >= model->desc.n_sa) return bad(": no such SA layer");
    if (model->device != ctx->device) return bad(": the model lives on another device");
    const pcr_pn2_msg_sa_desc& sd = model->desc.sa[layer];
    const uint32_t nb = sd.n_branch;
    if (!msg && nb != 1) return bad(": the layer has several branches (pcr_sa_msg_mlp_max_f32 runs them)");
    const bool ga = sd.group_all != 0;
    const size_t D = model->sa_in[layer] - 3, width = model->sa_out[layer];
    if (ga ? (centres || centre_seg_ptr || idx) : (!centres || !centre_seg_ptr)) return bad(": centres / centre_seg_ptr / idx go with a sampling layer only");
    if (D > 0 && !features) return bad(": the layer takes features");
    if (n_seg > PN_MAX_ROWS || cloud->n > PN_MAX_ROWS || (centres && centres->n > PN_MAX_ROWS)) return bad(": too large");
    if (!seg_ok(seg_ptr, n_seg, cloud->n) || (!ga && !seg_ok(centre_seg_ptr, n_seg, centres->n))) return bad(": seg_ptr must ascend and end inside its cloud");
    if (n_seg == 0) return PCR_OK;
    const size_t q0 = ga ? 0 : centre_seg_ptr[0], nq = ga ? n_seg : centre_seg_ptr[n_seg] - q0;
    const size_t p0 = seg_ptr[0], np = seg_ptr[n_seg] - p0;
    if (nq == 0) return PCR_OK;
    if (!out || (!ga && !idx)) return bad(": idx / out is NULL");
    size_t row_total = 0;                                        // entries of idx per centre, over the branches
    for (uint32_t b = 0; b < nb; b++) row_total += ga ? 0 : sd.branch[b].nsample;
    if ((ga ? (unsigned long long)np : (unsigned long long)nq * row_total) > PN_MAX_ROWS || nq > PN_MAX_ROWS / width) return bad(": too large");
    const bool compact = !ga && compact_rows(ctx, model->compact_default);
    std::vector<uint32_t> cs, rp;                                // the segment of every centre; compacted: per branch the nq + 1 row offsets
    if (!ga) {
        cs.resize(centre_seg_ptr[n_seg]);
        for (size_t s = 0; s < n_seg; s++)
            for (uint32_t q = centre_seg_ptr[s]; q < centre_seg_ptr[s + 1]; q++) cs[q] = (uint32_t)s;
        if (compact) rp.resize((size_t)nb * (nq + 1));
        size_t off = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const size_t nsample = sd.branch[b].nsample;
            uint32_t run = 0;
            for (size_t q = 0; q < nq; q++) {
                const uint32_t sg = cs[q0 + q], n = seg_ptr[sg + 1] - seg_ptr[sg];
                const uint32_t* row = idx + off + q * nsample;
                size_t inside = 0, last = 0;                     // entries inside the segment; the last entry that differs from the first
                for (size_t k = 0; k < nsample; k++) {
                    if (row[k] < n) inside++;
                    else if (!msg || row[k] != n) return bad(": an index lies outside its segment (an empty ball-query row?)");
                    if (row[k] != row[0]) last = k;
                }
                if (inside != 0 && inside != nsample) return bad(": an index lies outside its segment (an empty ball-query row?)");
                if (compact) { rp[(size_t)b * (nq + 1) + q] = run; run += inside ? (uint32_t)(last + 1) : 0u; }
            }
            if (compact) rp[(size_t)b * (nq + 1) + nq] = run;
            off += nq * nsample;
        }
    }
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *seg_dev, *cs_dev, *idx_dev, *rp_dev;
    float *feat_dev, *out_dev;
    Layout L;
    L.add(&seg_dev, n_seg + 1);
    L.add(&cs_dev, cs.size());
    L.add(&idx_dev, nq * row_total);
    L.add(&rp_dev, rp.size());
    L.add(&feat_dev, np * D);
    L.add(&out_dev, nq * width);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg_ptr, (n_seg + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!ga) {
        PCR_HIP(ctx, hipMemcpyAsync(cs_dev, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        PCR_HIP(ctx, hipMemcpyAsync(idx_dev, idx, nq * row_total * 4, hipMemcpyHostToDevice, ctx->stream));
        if (compact) PCR_HIP(ctx, hipMemcpyAsync(rp_dev, rp.data(), rp.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (D && np) PCR_HIP(ctx, hipMemcpyAsync(feat_dev, features + p0 * D, np * D * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    bool cleared = false;
    size_t off = 0;
    uint32_t col = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const Chain& ch = model->sa[layer][b];
        const size_t nsample = ga ? 1 : sd.branch[b].nsample;
        const unsigned long long rows = ga ? np : (unsigned long long)nq * nsample;
        ChainArgs a;
        memset(&a, 0, sizeof(a));
        a.x = cloud->x(); a.y = cloud->y(); a.z = cloud->z();
        if (!ga) {
            a.qx = centres->x() + q0; a.qy = centres->y() + q0; a.qz = centres->z() + q0; a.centre_seg = cs_dev + q0; a.idx = idx_dev + off;
            if (compact) a.row_ptr = rp_dev + (size_t)b * (nq + 1);
        }
        a.seg_ptr = seg_dev;
        a.feat = feat_dev - p0 * D;          // addressed by cloud position: moved back by the rows that were not uploaded (never dereferenced there)
        a.out = out_dev;
        a.out_stride = (uint32_t)width; a.out_col = col; a.xyz_last = sd.xyz_last;
        a.rows = (uint32_t)rows;
        a.D = (uint32_t)D; a.nsample = (uint32_t)nsample; a.n_seg = (uint32_t)n_seg; a.p0 = (uint32_t)p0;
        a.mode = ga ? PN2_GROUP_ALL : PN2_GROUPED;
        if (rows != 0) {
            rc = chain_launch(ctx, ch, a, nq, "pn2_sa", !cleared);
            if (rc) return rc;
            cleared = true;
        }
        off += nq * nsample;
        col += ch.n_out();
    }
    if (!cleared) PCR_HIP(ctx, hipMemsetAsync(out_dev, 0, nq * width * 4, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(out, out_dev, nq * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

}  // namespace

extern "C" int pcr_sa_mlp_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int layer, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres,
                                  const uint32_t* centre_seg_ptr, size_t n_seg, const float* features, const uint32_t* idx, float* out)
{
    return sa_layer(ctx, model, layer, cloud, seg_ptr, centres, centre_seg_ptr, n_seg, features, idx, out, false);
}

extern "C" int pcr_sa_msg_mlp_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int layer, const pcr_cloud* cloud, const uint32_t* seg_ptr, const pcr_cloud* centres,
                                      const uint32_t* centre_seg_ptr, size_t n_seg, const float* features, const uint32_t* idx, float* out)
{
    return sa_layer(ctx, model, layer, cloud, seg_ptr, centres, centre_seg_ptr, n_seg, features, idx, out, true);
}

// ---- the frame of a forward pass (pcr_pn2_forward_f32, pcr_pointnet_forward_f32): its checks, its upload, its tail -----------------------------------
namespace {

bool pn1_model_of(pcr_ctx* ctx, const pcr_pn2_model* model, const char* who)
{
    if (model->pn1) return true;
    fail(ctx, PCR_ERR_ARG, (std::string(who) + ": not a model of pcr_pn1_model_create").c_str());
    return false;
}

// the handles of a pass: there, of the entry point's kind (pn1: a model of pcr_pn1_model_create), on the context's device
int pass_model(pcr_ctx* ctx, const pcr_pn2_model* model, const char* who, bool pn1)
{
    if (!ctx || !model) return fail(ctx, PCR_ERR_ARG, who);
    if (pn1 && !pn1_model_of(ctx, model, who)) return PCR_ERR_ARG;
    if (!pn1 && model->pn1) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a model of pcr_pn1_model_create (pcr_pointnet_forward_f32 runs it)").c_str());
    if (model->device != ctx->device) return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": the model lives on another device").c_str());
    return PCR_OK;
}

// the arguments of a pass in their order of precedence (own_bad: the caller's own finding or NULL, behind npts); C0: floats per point.
// No objects is PCR_OK before objects and logp are looked at: the caller returns on rc != 0 OR n_obj == 0
int pass_args(pcr_ctx* ctx, const char* who, const char* own_bad, const float* objects, const float* logp, size_t n_obj, size_t npts, uint32_t C0)
{
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string(who) + what).c_str()); };
    if (npts < 1) return bad(": npts must be >= 1");
    if (own_bad) return bad(own_bad);
    if (n_obj == 0) return PCR_OK;
    if (!objects || !logp) return bad(": objects / logp is NULL");
    if (n_obj > PN_MAX_ROWS || npts > PN_MAX_ROWS || (unsigned long long)n_obj * npts > PN_MAX_ROWS / C0) return bad(": too large");
    return PCR_OK;
}

// the uploaded part of a pass: the objects split into x y z | features, the segment table of every cloud (cloud 0: the objects, N[0] points each; cloud l: the
// centres of sampling layer l - 1, N[l] each) and, for every cloud behind the first, the segment of each of its points
struct PassInput {
    Layout up;
    size_t P = 0;                               // points of cloud 0
    float *x0 = nullptr, *feat0 = nullptr;      // x, y, z one after the other, P floats each; P x D0
    uint32_t* seg[PCR_PN2_MAX_SA + 1];          // the segments of cloud l: n_obj + 1 offsets
    uint32_t* cseg[PCR_PN2_MAX_SA];             // the segment of every centre of sampling layer l (a point of cloud l + 1)

    void declare(size_t n_obj, const size_t* N, uint32_t n_clouds, uint32_t D0)
    {
        P = n_obj * N[0];
        up.add(&x0, 3 * P);
        up.add(&feat0, P * D0);
        for (uint32_t l = 0; l < n_clouds; l++) up.add(&seg[l], n_obj + 1);
        for (uint32_t l = 0; l + 1 < n_clouds; l++) up.add(&cseg[l], n_obj * N[l + 1]);
    }
};

// objects (P points of 3 + D0 floats) -> x, y, z (P floats each, one after the other at x0) and the features; false at the first value that is not finite.
// FEAT = false: D0 == 0 with a straight-line body, three checks and three stores per point (one generic loop cost pcr_pointnet_forward_f32 0.6 ns per point)
template <bool FEAT>
bool stage_points(const float* objects, size_t P, uint32_t D0, float* x0, float* feat0)
{
    float *hx = x0, *hy = x0 + P, *hz = x0 + 2 * P;
    const uint32_t C0 = FEAT ? 3 + D0 : 3;
    for (size_t i = 0; i < P; i++) {
        const float* r = objects + i * C0;
        if (!(fabsf(r[0]) <= FLT_MAX) || !(fabsf(r[1]) <= FLT_MAX) || !(fabsf(r[2]) <= FLT_MAX)) return false;
        hx[i] = r[0]; hy[i] = r[1]; hz[i] = r[2];
        if (FEAT)
            for (uint32_t c = 0; c < D0; c++) {
                if (!(fabsf(r[3 + c]) <= FLT_MAX)) return false;
                feat0[i * D0 + c] = r[3 + c];
            }
    }
    return true;
}

// one scratch block for `in.up` and the layouts `behind` it, back to back; every coordinate and feature checked on its way into the pinned staging block,
// the tables written there in the same layout; everything bound to the scratch block; the one upload
int pass_upload(pcr_ctx* ctx, const char* who, PassInput& in, const std::vector<const Layout*>& behind, const float* objects, size_t n_obj, const size_t* N,
                uint32_t n_clouds, uint32_t D0)
{
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    size_t total = in.up.bytes();
    for (const Layout* L : behind) total += L->bytes();
    int rc = ensure_scratch(ctx, total);
    if (rc) return rc;
    rc = ensure_stage(ctx, in.up.bytes());
    if (rc) return rc;
    in.up.bind(ctx->host_stage);
    if (!(D0 ? stage_points<true>(objects, in.P, D0, in.x0, in.feat0) : stage_points<false>(objects, in.P, 0, in.x0, in.feat0)))
        return fail(ctx, PCR_ERR_ARG, (std::string(who) + ": a non-finite coordinate or feature").c_str());
    for (uint32_t l = 0; l < n_clouds; l++)
        for (size_t o = 0; o <= n_obj; o++) in.seg[l][o] = (uint32_t)(o * N[l]);
    for (uint32_t l = 0; l + 1 < n_clouds; l++)
        for (size_t q = 0; q < n_obj * N[l + 1]; q++) in.cseg[l][q] = (uint32_t)(q / N[l + 1]);
    char* p = (char*)ctx->scratch;
    in.up.bind(p);
    p += in.up.bytes();
    for (const Layout* L : behind) { L->bind(p); p += L->bytes(); }
    PCR_HIP(ctx, hipMemcpyAsync(ctx->scratch, ctx->host_stage, in.up.bytes(), hipMemcpyHostToDevice, ctx->stream));
    return PCR_OK;
}

struct Download { void* dst; const void* src; size_t bytes; };      // dst NULL: not wanted

// the buffers of a pass's tail: the last slots of its last Layout
struct PassTail {
    float *logits = nullptr, *logp = nullptr;
    int32_t* pred = nullptr;
    void declare(Layout& L, size_t n_obj, uint32_t n_class)
    {
        L.add(&logits, n_obj * n_class);
        L.add(&logp, n_obj * n_class);
        L.add(&pred, n_obj);
    }
};

// the tail of a pass: the global feature (n_obj x c_last) through the head, log_softmax, logp and `more` to the host, the one wait, rc before the HIP error
int pass_tail(pcr_ctx* ctx, const char* who, int rc, const pcr_pn2_model* model, const float* gfeat, uint32_t c_last, size_t n_obj, const PassTail& t, float* logp,
              const std::vector<Download>& more)
{
    const uint32_t n_class = model->head.n_out();
    if (rc == PCR_OK) rc = head_launch(ctx, model->head, gfeat, c_last, t.logits, n_obj);
    hipError_t e = hipSuccess;
    if (rc == PCR_OK) {
        {
            ProfScope ps(ctx, "pn2_logsoftmax");
            hipLaunchKernelGGL(pn2_logsoftmax_kernel, dim3((unsigned)((n_obj + PN2_BLOCK - 1) / PN2_BLOCK)), dim3(PN2_BLOCK), 0, ctx->stream, t.logits, (uint32_t)n_obj, n_class,
                               t.logp, t.pred);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(logp, t.logp, n_obj * n_class * 4, hipMemcpyDeviceToHost, ctx->stream);
        for (const Download& d : more)
            if (e == hipSuccess && d.dst) e = hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);      // the one wait: the staging block (and the SSG / MSG pass's FPS jobs) are read until here
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(ctx, PCR_ERR_HIP, who, e != hipSuccess ? e : e2);
    prof_flush(ctx);
    return PCR_OK;
}

}  // namespace

extern "C" int pcr_pn2_forward_f32(pcr_ctx* ctx, const pcr_pn2_model* model, const float* objects, size_t n_obj, size_t npts, const uint32_t* starts, uint64_t seed,
                                   float* logp, int32_t* pred, float* global_feat, uint32_t* fps_idx)
{
    const char* who = "pcr_pn2_forward_f32";
    int rc = pass_model(ctx, model, who, false);
    if (rc) return rc;
    const pcr_pn2_msg_desc& d = model->desc;
    if (!d.sa[d.n_sa - 1].group_all) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_forward_f32: the last SA layer must be group_all");
    const uint32_t ns = model->n_sampling, D0 = d.D0;
    rc = pass_args(ctx, who, nullptr, objects, logp, n_obj, npts, 3 + D0);
    if (rc || n_obj == 0) return rc;
    const uint32_t n_class = model->head.n_out(), c_last = model->sa_out[d.n_sa - 1];
    const bool compact = compact_rows(ctx, model->compact_default);
    // ---- sizes of every stage
    size_t N[PCR_PN2_MAX_SA + 1];
    N[0] = npts;
    for (uint32_t l = 0; l < ns; l++) {
        const pcr_pn2_msg_sa_desc& s = d.sa[l];
        N[l + 1] = s.npoint;
        const unsigned long long nq = (unsigned long long)n_obj * s.npoint;
        unsigned long long row_total = 0;
        for (uint32_t b = 0; b < s.n_branch; b++) row_total += s.branch[b].nsample;
        if (nq > PN_MAX_ROWS / row_total || nq > PN_MAX_ROWS / model->sa_out[l]) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_forward_f32: too large");
    }
    if ((unsigned long long)n_obj * std::max<uint32_t>(c_last, n_class) > PN_MAX_ROWS) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_forward_f32: too large");
    std::vector<uint32_t> st((size_t)ns * n_obj);
    for (uint32_t l = 0; l < ns; l++)
        for (size_t o = 0; o < n_obj; o++) {
            uint32_t v;
            if (starts) {
                v = starts[(size_t)l * n_obj + o];
                if (v >= N[l]) return fail(ctx, PCR_ERR_ARG, "pcr_pn2_forward_f32: a start outside its object");
            } else {
                v = (uint32_t)(splitmix_key(seed, ((unsigned long long)(l + 1) << 32) | (unsigned long long)o) % (unsigned long long)N[l]);
            }
            st[(size_t)l * n_obj + o] = v;
        }
    // ---- one block: [uploaded: x y z feat | seg tables] [per sampling layer: picks, centres, ball rows, features out] [group_all out | head]
    PassInput in;
    in.declare(n_obj, N, ns + 1, D0);
    uint32_t *fps[PCR_PN2_MAX_SA], *bidx[PCR_PN2_MAX_SA][PCR_PN2_MAX_BRANCH], *bcnt[PCR_PN2_MAX_SA], *brp[PCR_PN2_MAX_SA];      // bcnt: n_branch x nq, brp: n_branch x (nq + 1)
    float *cxyz[PCR_PN2_MAX_SA], *sa_out[PCR_PN2_MAX_SA], *ga_out;
    Layout per[PCR_PN2_MAX_SA], last;
    std::vector<const Layout*> behind;          // one Layout per sampling layer, then the group_all layer's output and the tail
    for (uint32_t l = 0; l < ns; l++) {
        const size_t nq = n_obj * N[l + 1];
        per[l].add(&fps[l], nq);
        per[l].add(&cxyz[l], 3 * nq);
        for (uint32_t b = 0; b < d.sa[l].n_branch; b++) per[l].add(&bidx[l][b], nq * d.sa[l].branch[b].nsample);
        per[l].add(&bcnt[l], nq * d.sa[l].n_branch);
        per[l].add(&brp[l], compact ? (nq + 1) * d.sa[l].n_branch : 0);
        per[l].add(&sa_out[l], nq * model->sa_out[l]);
        behind.push_back(&per[l]);
    }
    PassTail tail;
    last.add(&ga_out, n_obj * c_last);
    tail.declare(last, n_obj, n_class);
    behind.push_back(&last);
    rc = pass_upload(ctx, who, in, behind, objects, n_obj, N, ns + 1, D0);
    if (rc) return rc;
    // ---- the sampling layers
    HostKeep keep;
    const size_t P = in.P;
    const float *cx = in.x0, *cy = in.x0 + P, *cz = in.x0 + 2 * P, *feat = in.feat0;
    uint32_t D = D0;
    for (uint32_t l = 0; l < ns; l++) {
        const pcr_pn2_msg_sa_desc& s = d.sa[l];
        const size_t nq = n_obj * N[l + 1];
        std::vector<FpsJob> jobs(n_obj);
        for (size_t o = 0; o < n_obj; o++) jobs[o] = { (uint32_t)(o * N[l]), (uint32_t)N[l], st[(size_t)l * n_obj + o], (uint32_t)o };
        rc = fps_device(ctx, cx, cy, cz, std::move(jobs), s.npoint, PCR_FPS_F32, fps[l], &keep);
        if (rc) break;
        float *qx = cxyz[l], *qy = qx + nq, *qz = qy + nq;
        {
            ProfScope ps(ctx, "pn2_centres");
            hipLaunchKernelGGL(pn2_centres_kernel, dim3((unsigned)((nq + PN2_BLOCK - 1) / PN2_BLOCK)), dim3(PN2_BLOCK), 0, ctx->stream, cx, cy, cz, fps[l], (uint32_t)N[l],
                               s.npoint, (uint32_t)nq, qx, qy, qz);
        }
        if (s.n_branch == 1) {
            rc = ball_query_device(ctx, cx, cy, cz, qx, qy, qz, in.seg[l], in.cseg[l], nq, s.branch[0].radius, s.branch[0].nsample, bidx[l][0], bcnt[l]);
        } else {                                 // every radius in one walk of the object
            double radii[PCR_PN2_MAX_BRANCH];
            uint32_t nsamples[PCR_PN2_MAX_BRANCH], *cb[PCR_PN2_MAX_BRANCH];
            for (uint32_t b = 0; b < s.n_branch; b++) { radii[b] = s.branch[b].radius; nsamples[b] = s.branch[b].nsample; cb[b] = bcnt[l] + (size_t)b * nq; }
            rc = ball_query_multi_device(ctx, cx, cy, cz, qx, qy, qz, in.seg[l], in.cseg[l], nq, s.n_branch, radii, nsamples, bidx[l], cb);
        }
        if (rc) break;
        if (compact) {                           // the row offsets of every branch: one launch
            rc = scan_launch(ctx, bcnt[l], nq, s.n_branch, brp[l]);
            if (rc) break;
        }
        uint32_t col = 0;
        for (uint32_t b = 0; b < s.n_branch && rc == PCR_OK; b++) {      // one chain per branch into its columns; the rows are cleared once
            ChainArgs a;
            memset(&a, 0, sizeof(a));
            a.x = cx; a.y = cy; a.z = cz; a.qx = qx; a.qy = qy; a.qz = qz;
            a.seg_ptr = in.seg[l]; a.centre_seg = in.cseg[l]; a.idx = bidx[l][b]; a.feat = feat; a.out = sa_out[l];
            if (compact) a.row_ptr = brp[l] + (size_t)b * (nq + 1);
            a.out_stride = model->sa_out[l]; a.out_col = col; a.xyz_last = s.xyz_last;
            a.rows = (uint32_t)(nq * s.branch[b].nsample);
            a.D = D; a.nsample = s.branch[b].nsample; a.n_seg = (uint32_t)n_obj; a.mode = PN2_GROUPED;
            rc = chain_launch(ctx, model->sa[l][b], a, nq, "pn2_sa", b == 0);
            col += model->sa[l][b].n_out();
        }
        if (rc) break;
        cx = qx; cy = qy; cz = qz; feat = sa_out[l];
        D = model->sa_out[l];
    }
    if (rc == PCR_OK) {                      // the group_all layer, then the head on its rows
        ChainArgs a;
        memset(&a, 0, sizeof(a));
        a.x = cx; a.y = cy; a.z = cz; a.seg_ptr = in.seg[ns]; a.feat = feat; a.out = ga_out;
        a.rows = (uint32_t)(n_obj * N[ns]);
        a.D = D; a.nsample = 1; a.n_seg = (uint32_t)n_obj; a.mode = PN2_GROUP_ALL; a.xyz_last = d.sa[ns].xyz_last;
        rc = chain_launch(ctx, model->sa[ns][0], a, n_obj, "pn2_sa");
    }
    std::vector<Download> more = { { pred, tail.pred, n_obj * 4 }, { global_feat, ga_out, n_obj * c_last * 4 } };
    size_t off = 0;
    for (uint32_t l = 0; l < ns && fps_idx; l++) {
        more.push_back({ fps_idx + off, fps[l], n_obj * N[l + 1] * 4 });
        off += n_obj * N[l + 1];
    }
    return pass_tail(ctx, who, rc, model, ga_out, c_last, n_obj, tail, logp, more);      // `keep` lives until its wait is over
}

// ---- the vanilla PointNet: model, stage entry point, forward pass ---------------------------------------------------------------------------------
namespace {

bool pn1_desc_info(const pcr_pn1_desc& d, size_t npts_hint, pcr_pn2_info* info)
{
    Pn1Layers ly;
    if (!pn1_layers(d, ly)) return false;
    const std::vector<LayerShape>& shapes = ly.shapes;
    memset(info, 0, sizeof(*info));
    info->n_weights = weight_count(shapes);
    info->n_class = d.fc_widths[d.n_fc - 1];
    info->c_last = d.widths[d.n_mlp - 1];
    uint64_t per_point = 0, per_object = 0;
    size_t i = 0;
    auto tnet = [&](uint32_t k) {
        for (uint32_t c = 0; c < 3; c++, i++) per_point += (uint64_t)shapes[i].K * shapes[i].N;
        for (uint32_t c = 0; c < 3; c++, i++) per_object += (uint64_t)shapes[i].K * shapes[i].N;
        per_point += (uint64_t)k * k;                     // the transform
    };
    if (d.stn3) tnet(3);
    for (uint32_t c = 0; c < d.n_mlp; c++, i++) per_point += (uint64_t)shapes[i].K * shapes[i].N;
    if (d.fstn) tnet(d.widths[0]);
    for (; i < shapes.size(); i++) per_object += (uint64_t)shapes[i].K * shapes[i].N;
    info->macs_per_object = per_point * npts_hint + per_object;
    return true;
}

}  // namespace

extern "C" int pcr_pn1_model_create(pcr_ctx* ctx, const pcr_pn1_desc* desc, const float* weights, size_t n_weights, pcr_pn2_model** out)
{
    if (out) *out = nullptr;
    if (!ctx || !desc || !weights || !out) return fail(ctx, PCR_ERR_ARG, "pcr_pn1_model_create");
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string("pcr_pn1_model_create") + what).c_str()); };
    Pn1Layers ly;
    if (!pn1_layers(*desc, ly)) return bad(": a descriptor outside the limits (see include/pcr.h)");
    std::unique_ptr<pcr_pn2_model> m;        // an error path below frees the device block with it
    std::vector<LayerDev> layer;
    const int rc = model_upload(ctx, "pcr_pn1_model_create", "pointnet", ly.shapes, weights, n_weights, desc->bn_eps, m, layer);
    if (rc) return rc;
    m->pn1 = true;
    m->d1 = *desc;
    // ---- the stages and the heads over the layers
    const size_t stn0 = ly.stn_first, enc0 = ly.enc_first, fstn0 = ly.fstn_first, head0 = ly.head_first;
    auto tnet_head = [&](Chain& ch, size_t first) {
        ch.n = 3;
        for (uint32_t k = 0; k < 3; k++) ch.L[k] = layer[first + 3 + k];
        lds_strides(ch);
    };
    if (desc->stn3) {
        Pn1Stage& st = m->stage[0];
        for (uint32_t k = 0; k < 3; k++) st.L[st.n++] = layer[stn0 + k];
        tnet_head(m->tnet_head[0], stn0);
    }
    if (desc->fstn) {
        Pn1Stage& st = m->stage[1];
        st.L[st.n++] = layer[enc0];
        for (uint32_t k = 0; k < 3; k++) st.L[st.n++] = layer[fstn0 + k];
        tnet_head(m->tnet_head[1], fstn0);
    }
    {
        Pn1Stage& st = m->stage[2];
        st.L[st.n++] = layer[enc0];
        if (desc->fstn) {
            LayerDev T;
            T.w = T.b = nullptr;
            T.K = T.N = desc->widths[0]; T.Kpad = T.Npad = pad16(desc->widths[0]);
            st.t_step = st.n;
            st.L[st.n++] = T;
        }
        for (uint32_t k = 1; k < desc->n_mlp; k++) st.L[st.n++] = layer[enc0 + k];
        st.relu_last = 0;
    }
    for (Pn1Stage& st : m->stage) {
        lds_strides(st);
        if (st.n && st.lds_bytes(16) > PN2_LDS_LIMIT) return bad(": a stage does not fit in LDS at 16 rows (see include/pcr.h)");
    }
    m->head.n = desc->n_fc;
    for (uint32_t k = 0; k < m->head.n; k++) m->head.L[k] = layer[head0 + k];
    lds_strides(m->head);
    if (m->head.lds_bytes(16) > PN2_LDS_LIMIT || (desc->stn3 && m->tnet_head[0].lds_bytes(16) > PN2_LDS_LIMIT) || (desc->fstn && m->tnet_head[1].lds_bytes(16) > PN2_LDS_LIMIT))
        return bad(": a head does not fit in LDS at 16 rows (see include/pcr.h)");
    *out = m.release();
    return PCR_OK;
}

extern "C" int pcr_pn1_model_info(const pcr_pn2_model* model, size_t npts_hint, pcr_pn2_info* info, pcr_pn1_desc* desc)
{
    if (!model) {                            // no model: *desc is READ, info is what a model made from it would report (no device needed)
        if (!desc || !info) return PCR_ERR_ARG;
        return pn1_desc_info(*desc, npts_hint, info) ? PCR_OK : PCR_ERR_ARG;
    }
    if (!model->pn1) return PCR_ERR_ARG;
    if (desc) *desc = model->d1;
    if (info) (void)pn1_desc_info(model->d1, npts_hint, info);
    return PCR_OK;
}

extern "C" int pcr_pointwise_chain_max_f32(pcr_ctx* ctx, const pcr_pn2_model* model, int stage, const pcr_cloud* cloud, const uint32_t* seg_ptr, size_t n_seg,
                                           const float* features, const float* trans3, const float* trans_feat, float* out)
{
    auto bad = [&](const char* what) { return fail(ctx, PCR_ERR_ARG, (std::string("pcr_pointwise_chain_max_f32") + what).c_str()); };
    if (!ctx || !model || !cloud || !seg_ptr) return bad("");
    if (!pn1_model_of(ctx, model, "pcr_pointwise_chain_max_f32")) return PCR_ERR_ARG;
    if (stage < 0 || stage > 2 || model->stage[stage].n == 0) return bad(": the model has no such stage");
    if (model->device != ctx->device) return bad(": the model lives on another device");
    const Pn1Stage& st = model->stage[stage];
    const size_t D = model->d1.D0, width = st.n_out(), K = model->d1.widths[0];
    const bool has_t = st.t_step < st.n;
    if (D > 0 && !features) return bad(": the model takes features");
    if (stage == 0 && trans3) return bad(": stage 0 takes no transform");
    if (has_t ? !trans_feat : trans_feat != nullptr) return bad(": trans_feat goes with stage 2 of a model with a feature T-Net, and only with it");
    if (n_seg > PN_MAX_ROWS || cloud->n > PN_MAX_ROWS) return bad(": too large");
    if (!seg_ok(seg_ptr, n_seg, cloud->n)) return bad(": seg_ptr must ascend and end inside its cloud");
    if (n_seg == 0) return PCR_OK;
    if (!out) return bad(": out is NULL");
    if (n_seg > PN_MAX_ROWS / width || (has_t && n_seg > PN_MAX_ROWS / (K * K))) return bad(": too large");
    const size_t p0 = seg_ptr[0], np = seg_ptr[n_seg] - p0;
    size_t max_pts = 0;
    for (size_t s = 0; s < n_seg; s++) max_pts = std::max<size_t>(max_pts, seg_ptr[s + 1] - seg_ptr[s]);
    PCR_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *seg_dev, *out_dev;
    float *feat_dev, *t3_dev, *tk_dev;
    Layout L;
    L.add(&seg_dev, n_seg + 1);
    L.add(&feat_dev, np * D);
    L.add(&t3_dev, trans3 ? n_seg * 9 : 0);
    L.add(&tk_dev, has_t ? n_seg * K * K : 0);
    L.add(&out_dev, n_seg * width);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(seg_dev, seg_ptr, (n_seg + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (D && np) PCR_HIP(ctx, hipMemcpyAsync(feat_dev, features + p0 * D, np * D * 4, hipMemcpyHostToDevice, ctx->stream));
    if (trans3) PCR_HIP(ctx, hipMemcpyAsync(t3_dev, trans3, n_seg * 9 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (has_t) PCR_HIP(ctx, hipMemcpyAsync(tk_dev, trans_feat, n_seg * K * K * 4, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));           // the caller's arrays are pageable: read before the call returns control to the launches
    Pn1Args a;
    memset(&a, 0, sizeof(a));
    a.x = cloud->x(); a.y = cloud->y(); a.z = cloud->z();
    a.feat = feat_dev - p0 * D;              // addressed by cloud position: moved back by the rows that were not uploaded (never dereferenced there)
    a.seg_ptr = seg_dev;
    a.trans3 = trans3 ? t3_dev : nullptr;
    a.transK = has_t ? tk_dev : nullptr;
    a.out = out_dev;
    a.D = (uint32_t)D;
    rc = pn1_launch(ctx, st, a, n_seg, max_pts);
    if (rc) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(out, out_dev, n_seg * width * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
    return PCR_OK;
}

extern "C" int pcr_pointnet_forward_f32(pcr_ctx* ctx, const pcr_pn2_model* model, const float* objects, size_t n_obj, size_t npts, float* logp, int32_t* pred,
                                        float* global_feat, float* trans, float* trans_feat)
{
    const char* who = "pcr_pointnet_forward_f32";
    int rc = pass_model(ctx, model, who, true);
    if (rc) return rc;
    const pcr_pn1_desc& d = model->d1;
    const uint32_t D0 = d.D0, K = d.widths[0], KK = K * K;
    rc = pass_args(ctx, who, (trans && !d.stn3) || (trans_feat && !d.fstn) ? ": the model has no such T-Net" : nullptr, objects, logp, n_obj, npts, 3 + D0);
    if (rc || n_obj == 0) return rc;
    const uint32_t n_class = model->head.n_out(), c_last = model->stage[2].n_out(), c_tnet = (d.stn3 || d.fstn) ? d.tnet_conv[2] : 0;
    if ((unsigned long long)n_obj * std::max(std::max(c_last, n_class), std::max(c_tnet, d.fstn ? KK : 0u)) > PN_MAX_ROWS)
        return fail(ctx, PCR_ERR_ARG, "pcr_pointnet_forward_f32: too large");
    // ---- one block: [uploaded: x y z | features | segments] [the T-Nets' pooled rows, trans, trans_feat | global feature | head]
    PassInput in;
    in.declare(n_obj, &npts, 1, D0);
    float *t3, *tk;
    uint32_t *pooled, *gf;                   // pooled / gf: keys while their chain runs, floats once it is decoded
    Layout L;
    L.add(&pooled, n_obj * c_tnet);          // both T-Nets pool into it, one after the other
    L.add(&t3, d.stn3 ? n_obj * 9 : 0);
    L.add(&tk, d.fstn ? n_obj * KK : 0);
    L.add(&gf, n_obj * c_last);
    PassTail tail;
    tail.declare(L, n_obj, n_class);
    rc = pass_upload(ctx, who, in, { &L }, objects, n_obj, &npts, 1, D0);
    if (rc) return rc;
    const size_t P = in.P;
    Pn1Args pa;
    memset(&pa, 0, sizeof(pa));
    pa.x = in.x0; pa.y = in.x0 + P; pa.z = in.x0 + 2 * P; pa.feat = in.feat0; pa.seg_ptr = in.seg[0]; pa.D = D0;
    auto tnet = [&](const Chain& ch, float* to, uint32_t k) {                          // pooled rows -> the FC layers -> + identity
        int r = head_launch(ctx, ch, (const float*)pooled, c_tnet, to, n_obj);
        if (r) return r;
        ProfScope ps(ctx, "pn1_identity");
        hipLaunchKernelGGL(pn1_identity_kernel, dim3((unsigned)((n_obj * k + PN2_BLOCK - 1) / PN2_BLOCK)), dim3(PN2_BLOCK), 0, ctx->stream, to, (uint32_t)n_obj, k);
        PCR_HIP(ctx, hipGetLastError());
        return (int)PCR_OK;
    };
    if (d.stn3) {                            // the input T-Net on the raw points
        pa.out = pooled;
        rc = pn1_launch(ctx, model->stage[0], pa, n_obj, npts);
        if (rc == PCR_OK) rc = tnet(model->tnet_head[0], t3, 3);
        pa.trans3 = t3;
    }
    if (rc == PCR_OK && d.fstn) {            // the feature T-Net on convolution 0 of the transformed points
        pa.out = pooled;
        rc = pn1_launch(ctx, model->stage[1], pa, n_obj, npts);
        if (rc == PCR_OK) rc = tnet(model->tnet_head[1], tk, K);
        pa.transK = tk;
    }
    if (rc == PCR_OK) {
        pa.out = gf;
        rc = pn1_launch(ctx, model->stage[2], pa, n_obj, npts);
    }
    return pass_tail(ctx, who, rc, model, (const float*)gf, c_last, n_obj, tail, logp,
                     { { pred, tail.pred, n_obj * 4 }, { global_feat, gf, n_obj * c_last * 4 }, { trans, t3, n_obj * 9 * 4 }, { trans_feat, tk, (size_t)n_obj * KK * 4 } });
}
