// range_image.hip — Homework4's second foreground path on the GPU: Homework4/foreground_clustering_range.py, pcd_to_range_image
// (:13-48), range_image_labeling (:51-95), cluster_assignment (:124-133) and depth_completion (:136-149).  Contracts: include/pcr.h.
//
// Projection — one lane per point, f64 on the f32 coordinates widened: d = sqrt((x*x + y*y) + z*z), alpha = atan2(y, x),
// beta = atan2(z, sqrt(x*x + y*y)) (DIFFERS: :34 calls math.asin with two arguments and cannot run), pixel = size - 1 - (floor(angle /
// res_rad) + ceil(size / 2)) per axis, an index in [-size, 0) wrapped as numpy does, anything else dropped.  The winner of a pixel is
// its highest point index (`range_image[y, x] = d[i]` in index order): a 32-bit atomicMax.
//   project  pixel of every point in the FULL image, winner[pixel] = max index, drop flags
//   fill     row / column occupancy flags of the full image (plain stores of 1)
//   crop     exclusive scans of the two flag rows (grid.hip's device scan), then compact: the cropped f64 image (d[winner] or -1)
//            and, per point, its pixel in the cropped image
// Labelling — connected components of the cropped image under the reference's edge test, which is symmetric in the two pixels:
//   union    one workgroup per RI_TH x RI_TW tile, staged in LDS with a halo of nn_mode rows below and nn_mode wrapped columns on
//            either side; every occupied pixel tests the FORWARD half of its window (later rows, and its own row at column offsets
//            +1 .. +nn_mode modulo cols), so each unordered pair is tested once, and links through union_find.hpp
//   flatten  full pointer jumping (parent[] only read): root[p] = the component's smallest raster index
//   label    flag[p] = occupied && root[p] == p, exclusive scan = ids in raster order of each component's first pixel
// Closing — dilation then erosion over a (2 pad + 1)^2 window from an LDS tile, the `pad` border left at -1.
// Every loop is bounded by the window, the tile or the pixel count; there is no ticket counter and no spin wait.
#include "pcr_internal.hpp"
#include "union_find.hpp"

#include <algorithm>
#include <cmath>
#include <new>

#pragma clang fp contract(off)

namespace pcr {

namespace {

constexpr int RI_BLOCK = 256;
constexpr int RI_TH = 16, RI_TW = 16;                   // tile of the union and closing kernels: one lane per pixel
constexpr int RI_NN_MAX = 8;                            // largest nn_mode (pcr.h)
constexpr int RI_PAD_MAX = 16;                          // largest pad of the closing (pcr.h)

struct RiGeom {
    int width, height;                                  // full image
    double off_w, off_h;                                // ceil(size / 2)
    double res_rad;
};

// pixel index along one axis, or -1 where numpy would raise IndexError
__device__ __forceinline__ int ri_axis(double angle, double res_rad, double off, int size)
{
    const double t = (double)(size - 1) - (floor(angle / res_rad) + off);
    if (!(t >= -(double)size && t < (double)size)) return -1;
    const int i = (int)t;
    return i < 0 ? i + size : i;
}

__global__ __launch_bounds__(RI_BLOCK) void ri_project_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                              uint32_t n, RiGeom g, double* __restrict__ d, int32_t* __restrict__ pixfull,
                                                              uint32_t* __restrict__ dropflag, int32_t* winner)
{
    const uint32_t i = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double px = x[i], py = y[i], pz = z[i];
    int pix = -1;
    double di = -1.0;
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
        const double h2 = px * px + py * py;
        di = sqrt(h2 + pz * pz);
        const double alpha = atan2(py, px);
        const double beta = atan2(pz, sqrt(h2));
        const int c = ri_axis(alpha, g.res_rad, g.off_w, g.width);
        const int r = ri_axis(beta, g.res_rad, g.off_h, g.height);
        if (c >= 0 && r >= 0) pix = r * g.width + c;
    }
    d[i] = di;
    pixfull[i] = pix;
    dropflag[i] = pix < 0 ? 1u : 0u;
    if (pix >= 0) atomicMax(winner + pix, (int32_t)i);
}

__global__ __launch_bounds__(RI_BLOCK) void ri_fill_kernel(const int32_t* __restrict__ winner, uint32_t npix, int width, uint32_t* rowflag,
                                                           uint32_t* colflag)
{
    const uint32_t p = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (p >= npix || winner[p] < 0) return;
    rowflag[p / (uint32_t)width] = 1u;
    colflag[p % (uint32_t)width] = 1u;
}

// the cropped image: a surviving row and column of the full image -> (rowmap, colmap)
__global__ __launch_bounds__(RI_BLOCK) void ri_compact_kernel(const int32_t* __restrict__ winner, const double* __restrict__ d, uint32_t npix, int width,
                                                              const uint32_t* __restrict__ rowflag, const uint32_t* __restrict__ colflag,
                                                              const uint32_t* __restrict__ rowmap, const uint32_t* __restrict__ colmap, int cols,
                                                              double* __restrict__ image)
{
    const uint32_t p = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const uint32_t r = p / (uint32_t)width, c = p % (uint32_t)width;
    if (!rowflag[r] || !colflag[c]) return;
    const int32_t w = winner[p];
    image[(size_t)rowmap[r] * cols + colmap[c]] = w >= 0 ? d[w] : -1.0;
}

__global__ __launch_bounds__(RI_BLOCK) void ri_remap_kernel(const int32_t* __restrict__ pixfull, uint32_t n, int width, const uint32_t* __restrict__ rowmap,
                                                            const uint32_t* __restrict__ colmap, int cols, int32_t* __restrict__ pix)
{
    const uint32_t i = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t p = pixfull[i];
    pix[i] = p < 0 ? -1 : (int32_t)(rowmap[p / width] * (uint32_t)cols + colmap[p % width]);
}

__global__ __launch_bounds__(RI_BLOCK) void ri_init_kernel(uint32_t* __restrict__ parent, uint32_t npix)
{
    const uint32_t p = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (p < npix) parent[p] = p;
}

struct RiEdge {
    double sphi, cphi;                                  // sin / cos of phi, taken on the host (the reference's libm)
    double thr;                                         // theta in radians
    double tan_lo, tan_hi;                              // tan(thr) (1 -+ 1e-9) while pre != 0
    int pre;
};

// the reference's test (:80-89) on two occupied pixels
__device__ __forceinline__ bool ri_edge(double a, double b, const RiEdge& e)
{
    const double d1 = fmax(a, b), d2 = fmin(a, b);
    if (!(fabs(d1 - d2) < 1.0)) return false;
    const double yy = d2 * e.sphi, xx = d1 - d2 * e.cphi;
    if (e.pre) {
        // 1e-3 <= thr <= 1.5: a relative distance of 1e-9 between yy / xx and tan(thr) is at least 7e-14 rad between the angle and thr,
        // against the 8 ulp (< 3e-15 rad) band of pcr.h; pairs nearer than that go to atan2
        if (!(yy > 0.0)) { if (yy <= 0.0) return false; }          // angle <= 0 < thr (NaN falls through to atan2)
        else if (xx <= 0.0) return true;                            // angle >= pi/2 > thr
        else if (yy > xx * e.tan_hi) return true;
        else if (yy < xx * e.tan_lo) return false;
    }
    return atan2(yy, xx) > e.thr;
}

__global__ __launch_bounds__(RI_BLOCK) void ri_union_kernel(const double* __restrict__ image, int rows, int cols, int nn, RiEdge e, uint32_t* parent,
                                                            uint32_t* err)
{
    constexpr int LW = RI_TW + 2 * RI_NN_MAX, LH = RI_TH + RI_NN_MAX;
    __shared__ double tile[LH][LW];
    const int r0 = blockIdx.y * RI_TH, c0 = blockIdx.x * RI_TW;
    const int lw = RI_TW + 2 * nn, lh = RI_TH + nn;
    for (int t = threadIdx.x; t < lh * lw; t += RI_BLOCK) {
        const int lr = t / lw, lc = t % lw;
        const int gr = r0 + lr;
        int gc = c0 - nn + lc;
        if (gc < 0) gc += cols;                             // wrapped once, as the reference does (:74-77)
        else if (gc >= cols) gc -= cols;
        tile[lr][lc] = (gr < rows && gc >= 0 && gc < cols) ? image[(size_t)gr * cols + gc] : -1.0;
    }
    __syncthreads();
    const int ty = threadIdx.x / RI_TW, tx = threadIdx.x % RI_TW;
    const int r = r0 + ty, c = c0 + tx;
    if (r >= rows || c >= cols) return;
    const double v = tile[ty][tx + nn];
    if (!(v > 0.0)) return;
    const uint32_t npix = (uint32_t)rows * (uint32_t)cols;
    const uint32_t p = (uint32_t)r * cols + c;
    uint32_t rp = p;                                        // an ancestor of p (refreshed by every find)
    for (int dr = 0; dr <= nn; dr++) {
        if (r + dr >= rows) break;
        for (int dc = dr ? -nn : 1; dc <= nn; dc++) {
            const double w = tile[ty + dr][tx + nn + dc];
            if (!(w > 0.0) || !ri_edge(v, w, e)) continue;
            int cn = c + dc;
            if (cn < 0) cn += cols;
            else if (cn >= cols) cn -= cols;
            const uint32_t q = (uint32_t)(r + dr) * cols + cn;
            if (q == p) continue;                           // cols <= nn: the window meets its own centre
            rp = uf_find(parent, rp, npix, err);
            const uint32_t rq = uf_find(parent, q, npix, err);
            if (rp != rq) uf_union(parent, rp, rq, npix, err);
        }
    }
}

// full pointer jumping (no hook can happen any more); parent[] is only read, as in db_final_kernel
__global__ __launch_bounds__(RI_BLOCK) void ri_flatten_kernel(const double* __restrict__ image, uint32_t npix, uint32_t* parent, uint32_t* __restrict__ root,
                                                              uint32_t* __restrict__ flag, uint32_t* err)
{
    const uint32_t p = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const uint32_t rt = uf_find<false>(parent, p, npix, err);
    root[p] = rt;
    flag[p] = (image[p] > 0.0 && rt == p) ? 1u : 0u;
}

__global__ __launch_bounds__(RI_BLOCK) void ri_label_kernel(const double* __restrict__ image, uint32_t npix, const uint32_t* __restrict__ root,
                                                            const uint32_t* __restrict__ ids, int32_t* __restrict__ label)
{
    const uint32_t p = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (p >= npix) return;
    label[p] = image[p] > 0.0 ? (int32_t)ids[root[p]] : -1;
}

__global__ __launch_bounds__(RI_BLOCK) void ri_assign_kernel(const int32_t* __restrict__ pix, uint32_t n, const int32_t* __restrict__ label,
                                                             int32_t* __restrict__ cluster_idx)
{
    const uint32_t i = blockIdx.x * RI_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t p = pix[i];
    cluster_idx[i] = p < 0 ? -1 : label[p];
}

// np.amax / np.amin keep a NaN once they have met one
template <bool MAX>
__device__ __forceinline__ double ri_pick(double m, double v)
{
    return ((MAX ? v > m : v < m) || v != v) ? v : m;
}

// out[r, c] = max (MAX) or min over in[r - pad .. r + pad, c - pad .. c + pad] for pad <= r < rows - pad, pad <= c < cols - pad, else -1
template <bool MAX>
__global__ __launch_bounds__(RI_BLOCK) void ri_close_kernel(const double* __restrict__ in, int rows, int cols, int pad, double* __restrict__ out)
{
    constexpr int LS = RI_TW + 2 * RI_PAD_MAX;
    __shared__ double tile[RI_TH + 2 * RI_PAD_MAX][LS];
    const int r0 = blockIdx.y * RI_TH, c0 = blockIdx.x * RI_TW;
    const int lw = RI_TW + 2 * pad, lh = RI_TH + 2 * pad;
    for (int t = threadIdx.x; t < lh * lw; t += RI_BLOCK) {
        const int lr = t / lw, lc = t % lw;
        const int gr = r0 - pad + lr, gc = c0 - pad + lc;
        tile[lr][lc] = (gr >= 0 && gr < rows && gc >= 0 && gc < cols) ? in[(size_t)gr * cols + gc] : -1.0;   // (never read by an inner pixel)
    }
    __syncthreads();
    const int ty = threadIdx.x / RI_TW, tx = threadIdx.x % RI_TW;
    const int r = r0 + ty, c = c0 + tx;
    if (r >= rows || c >= cols) return;
    double m = -1.0;
    if (r >= pad && r < rows - pad && c >= pad && c < cols - pad) {
        m = tile[ty][tx];
        for (int dr = 0; dr <= 2 * pad; dr++)
            for (int dc = 0; dc <= 2 * pad; dc++) m = ri_pick<MAX>(m, tile[ty + dr][tx + dc]);
    }
    out[(size_t)r * cols + c] = m;
}

inline dim3 grid1(size_t n) { return dim3((unsigned)((n + RI_BLOCK - 1) / RI_BLOCK)); }
inline dim3 grid2(int rows, int cols) { return dim3((unsigned)((cols + RI_TW - 1) / RI_TW), (unsigned)((rows + RI_TH - 1) / RI_TH)); }

}  // namespace

int ri_alloc(pcr_ctx* ctx, size_t n_points, int rows, int cols, pcr_range_image** out)
{
    pcr_range_image* img = new (std::nothrow) pcr_range_image();
    if (!img) return fail(ctx, PCR_ERR_NOMEM, "pcr_range_image");
    img->n_points = n_points;
    img->rows = rows;
    img->cols = cols;
    const size_t npix = (size_t)rows * cols;
    hipError_t e = hipMalloc((void**)&img->image, std::max<size_t>(npix, 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&img->label, std::max<size_t>(npix, 1) * 4);
    if (e == hipSuccess && n_points) e = hipMalloc((void**)&img->pix, n_points * 4);
    if (e != hipSuccess) { ri_destroy(ctx, img); return fail(ctx, PCR_ERR_HIP, "pcr_range_image: hipMalloc", e); }
    *out = img;
    return PCR_OK;
}

int ri_destroy(pcr_ctx* ctx, pcr_range_image* img)
{
    if (!img) return PCR_OK;
    if (ctx && ctx->stream) hipStreamSynchronize(ctx->stream);
    if (img->image) hipFree(img->image);
    if (img->label) hipFree(img->label);
    if (img->pix) hipFree(img->pix);
    delete img;
    return PCR_OK;
}

int ri_create(pcr_ctx* ctx, const pcr_cloud* cloud, double resolution_deg, int width, int height, pcr_range_image** out)
{
    const size_t n = cloud->n;
    const size_t npix = (size_t)width * height;
    RiGeom g;
    g.width = width;
    g.height = height;
    g.off_w = std::ceil(width / 2.0);
    g.off_h = std::ceil(height / 2.0);
    g.res_rad = M_PI / 180 * resolution_deg;               // :19
    int32_t *winner, *pixfull;
    double* d;
    uint32_t *dropflag, *dropscan, *rowflag, *colflag, *rowmap, *colmap, *tot_rows, *tot_cols, *tot_drop, *grand;
    Layout L;
    L.add(&winner, npix);
    L.add(&d, n);
    L.add(&pixfull, n);
    L.add(&dropflag, n);
    L.add(&dropscan, n);
    L.add(&rowflag, height);
    L.add(&colflag, width);      // (directly behind rowflag: one memset clears both)
    L.add(&rowmap, height);
    L.add(&colmap, width);
    L.add(&tot_rows, scan_blocks(height));
    L.add(&tot_cols, scan_blocks(width));
    L.add(&tot_drop, scan_blocks(n));
    L.add(&grand, 3);            // [0] rows, [1] cols, [2] dropped points
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(winner, 0xFF, npix * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rowflag, 0, (char*)(colflag + width) - (char*)rowflag, ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_create_f32: memset", e);
    {
        ProfScope ps(ctx, "ri_project", 1);
        hipLaunchKernelGGL(ri_project_kernel, grid1(n), dim3(RI_BLOCK), 0, ctx->stream, cloud->x(), cloud->y(), cloud->z(), (uint32_t)n, g, d, pixfull,
                           dropflag, winner);
        hipLaunchKernelGGL(ri_fill_kernel, grid1(npix), dim3(RI_BLOCK), 0, ctx->stream, winner, (uint32_t)npix, width, rowflag, colflag);
    }
    e = hipGetLastError();
    uint32_t words[3] = { 0, 0, 0 };
    {
        ProfScope ps(ctx, "ri_crop", 1);
        if (e == hipSuccess && exclusive_scan_u32(ctx, rowflag, rowmap, height, tot_rows, grand + 0)) e = hipErrorUnknown;
        if (e == hipSuccess && exclusive_scan_u32(ctx, colflag, colmap, width, tot_cols, grand + 1)) e = hipErrorUnknown;
        if (e == hipSuccess && exclusive_scan_u32(ctx, dropflag, dropscan, n, tot_drop, grand + 2)) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipMemcpyAsync(words, grand, sizeof words, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_create_f32", e);
    if (words[0] == 0 || words[1] == 0) return fail(ctx, PCR_ERR_EMPTY, "pcr_range_image_create_f32: no point lands in the image");
    pcr_range_image* img = nullptr;
    rc = ri_alloc(ctx, n, (int)words[0], (int)words[1], &img);
    if (rc) return rc;
    img->full_rows = height;
    img->full_cols = width;
    img->dropped = words[2];
    {
        ProfScope ps(ctx, "ri_crop", 1);
        hipLaunchKernelGGL(ri_compact_kernel, grid1(npix), dim3(RI_BLOCK), 0, ctx->stream, winner, d, (uint32_t)npix, width, rowflag, colflag, rowmap, colmap,
                           img->cols, img->image);
        hipLaunchKernelGGL(ri_remap_kernel, grid1(n), dim3(RI_BLOCK), 0, ctx->stream, pixfull, (uint32_t)n, width, rowmap, colmap, img->cols, img->pix);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the scratch may be reused by the next call of any kind
    if (e != hipSuccess) { ri_destroy(ctx, img); return fail(ctx, PCR_ERR_HIP, "pcr_range_image_create_f32: crop", e); }
    prof_flush(ctx);
    *out = img;
    return PCR_OK;
}

int ri_from_host(pcr_ctx* ctx, const double* image, int rows, int cols, pcr_range_image** out)
{
    pcr_range_image* img = nullptr;
    int rc = ri_alloc(ctx, 0, rows, cols, &img);
    if (rc) return rc;
    img->full_rows = rows;
    img->full_cols = cols;
    hipError_t e = hipMemcpyAsync(img->image, image, (size_t)rows * cols * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ri_destroy(ctx, img); return fail(ctx, PCR_ERR_HIP, "pcr_range_image_from_host_f64", e); }
    *out = img;
    return PCR_OK;
}

int ri_read(pcr_ctx* ctx, const pcr_range_image* img, double* image, int32_t* pixel)
{
    hipError_t e = hipSuccess;
    if (image) e = hipMemcpyAsync(image, img->image, (size_t)img->rows * img->cols * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && pixel && img->n_points) e = hipMemcpyAsync(pixel, img->pix, img->n_points * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_read", e);
    return PCR_OK;
}

int ri_close(pcr_ctx* ctx, pcr_range_image* img, int pad)
{
    const size_t npix = (size_t)img->rows * img->cols;
    int rc = ensure_scratch(ctx, npix * 8);
    if (rc) return rc;
    double* dila = (double*)ctx->scratch;
    {
        ProfScope ps(ctx, "ri_close", 1);
        const dim3 g = grid2(img->rows, img->cols);
        hipLaunchKernelGGL(ri_close_kernel<true>, g, dim3(RI_BLOCK), 0, ctx->stream, img->image, img->rows, img->cols, pad, dila);
        hipLaunchKernelGGL(ri_close_kernel<false>, g, dim3(RI_BLOCK), 0, ctx->stream, dila, img->rows, img->cols, pad, img->image);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_close_f64", e);
    img->labelled = false;
    prof_flush(ctx);
    return PCR_OK;
}

int ri_label(pcr_ctx* ctx, pcr_range_image* img, double phi_deg, double theta_deg, int nn_mode, int32_t* image_label, uint64_t* n_labels)
{
    const size_t npix = (size_t)img->rows * img->cols;
    uint32_t *parent, *root, *flag, *ids, *totals, *n_ids, *err;
    Layout L;
    L.add(&parent, npix);
    L.add(&root, npix);
    L.add(&flag, npix);
    L.add(&ids, npix);
    L.add(&totals, scan_blocks(npix));
    L.add(&n_ids, 1);            // the scan's grand total: the number of labels
    L.add(&err, 1);
    int rc = bind_scratch(ctx, L);
    if (rc) return rc;
    RiEdge ed;
    const double phi = phi_deg * M_PI / 180;               // :52
    ed.thr = theta_deg * M_PI / 180;                       // :53
    ed.sphi = std::sin(phi);
    ed.cphi = std::cos(phi);
    ed.pre = (ed.thr >= 1e-3 && ed.thr <= 1.5 && tune_get(ctx, "ri_prefilter", 1) > 0) ? 1 : 0;     // tune ri_prefilter = -1: every pair goes to atan2
    const double tt = std::tan(ed.thr);
    ed.tan_lo = tt * (1.0 - 1e-9);
    ed.tan_hi = tt * (1.0 + 1e-9);
    hipError_t e = hipMemsetAsync(err, 0, 4, ctx->stream);
    {
        ProfScope ps(ctx, "ri_union", 1);
        hipLaunchKernelGGL(ri_init_kernel, grid1(npix), dim3(RI_BLOCK), 0, ctx->stream, parent, (uint32_t)npix);
        hipLaunchKernelGGL(ri_union_kernel, grid2(img->rows, img->cols), dim3(RI_BLOCK), 0, ctx->stream, img->image, img->rows, img->cols, nn_mode, ed,
                           parent, err);
    }
    {
        ProfScope ps(ctx, "ri_label", 1);
        hipLaunchKernelGGL(ri_flatten_kernel, grid1(npix), dim3(RI_BLOCK), 0, ctx->stream, img->image, (uint32_t)npix, parent, root, flag, err);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && exclusive_scan_u32(ctx, flag, ids, npix, totals, n_ids)) e = hipErrorUnknown;
        hipLaunchKernelGGL(ri_label_kernel, grid1(npix), dim3(RI_BLOCK), 0, ctx->stream, img->image, (uint32_t)npix, root, ids, img->label);
    }
    uint32_t words[2] = { 0, 0 };                           // error word, labels
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && image_label) e = hipMemcpyAsync(image_label, img->label, npix * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&words[0], err, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&words[1], n_ids, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_label_f64", e);
    prof_flush(ctx);
    if (words[0]) return fail(ctx, PCR_ERR_STATE, "pcr_range_image_label_f64: union-find bound exceeded (corrupt structure)");
    img->labelled = true;
    img->n_labels = words[1];
    if (n_labels) *n_labels = words[1];
    return PCR_OK;
}

int ri_assign(pcr_ctx* ctx, const pcr_range_image* img, int32_t* cluster_idx)
{
    const size_t n = img->n_points;
    if (n == 0) return PCR_OK;
    int rc = ensure_scratch(ctx, n * 4);
    if (rc) return rc;
    int32_t* out = (int32_t*)ctx->scratch;
    {
        ProfScope ps(ctx, "ri_assign", 1);
        hipLaunchKernelGGL(ri_assign_kernel, grid1(n), dim3(RI_BLOCK), 0, ctx->stream, img->pix, (uint32_t)n, img->label, out);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cluster_idx, out, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PCR_ERR_HIP, "pcr_range_image_assign", e);
    prof_flush(ctx);
    return PCR_OK;
}

}  // namespace pcr
