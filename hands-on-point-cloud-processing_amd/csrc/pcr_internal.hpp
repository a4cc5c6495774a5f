// pcr_internal.hpp — shared host-side declarations of libpcr_hip.so (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "pcr.h"
#include "scratch_layout.hpp"

namespace pcr {

// Every cloud is allocated with its length rounded up to PAD points; x of the padding is +inf so that a
// padded target can never win a nearest-neighbour comparison (d2 = +inf is not < FLT_MAX).
constexpr size_t PAD = 1024;
constexpr int PCR_NSTATS = 16;      // diagnostics words of a 1-NN launch (tune grid_stats; pcr_nn1_stats)
// the accumulators of the ICP sums + solve launch (kabsch.hip): replicas (a power of two) of 48 int64 = three 128-byte lines each
constexpr int ICP_ACC_REPLICAS = 8, ICP_ACC_WORDS = 48;
// ... of which there are two SETS: the chain sums -> search adds iteration k into set k & 1; every other user has set 0 alone
constexpr int ICP_ACC_SETS = 2;
// with a ticket per replica: the workgroups of a launch of `blocks` workgroups that arrive at replica r (workgroup b belongs to replica
// b & (R - 1)); 0 for a replica the launch does not reach, which nobody waits for
__host__ __device__ constexpr uint32_t icp_replica_members(uint32_t blocks, uint32_t r)
{
    return r < (uint32_t)ICP_ACC_REPLICAS && r < blocks ? (blocks - r + ICP_ACC_REPLICAS - 1) / ICP_ACC_REPLICAS : 0u;
}

inline size_t padded(size_t n) { return ((n + PAD - 1) / PAD) * PAD + PAD; }   // always >= 1 full pad block

struct ProfEntry {
    uint64_t launches = 0;
    double total_ms = 0.0;
    std::vector<float> each_ms;           // the individual durations since the last reset, in launch order (at most 4096 kept)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// device-resident state of the pipelined ICP loop (registration.cpp:910-1006); mirrored in pinned host memory
struct IcpState {
    float Rd[9];
    float td[3];
    float T_total[16];
    float last_loss;
    float loss;
    float eps;
    int converged;
    int empty;
    int stop;                    // set by the update kernel: later kernels of the stream become no-ops
    int stop_after_transform;    // max_iter reached: stop once the last transform has been applied
    int overflow;                // a kept source point lay beyond the fixed-point grid of the Kabsch sums (kabsch_plan): PCR_ERR_STATE
    int barrier_timeout;         // the workgroups of a fused sums + move launch did not meet within its bound (kabsch.hip): PCR_ERR_STATE
    unsigned long long unchanged;
    unsigned long long iters_run;
    unsigned long long max_iter;
    unsigned long long last_pairs;
};
// a slot of the pinned host ring the pipelined loop learns the state from (icp.cpp): the state, and behind it the sequence number of the launch that
// wrote it where the sums + solve launch stores the snapshot itself — seq only grows over a context's life, so a slot left by an
// earlier call or an earlier trip round the ring is never taken for the one awaited
struct IcpSnapSlot {
    IcpState state;
    unsigned long long seq;
};
// what a moving search that also finishes the previous iteration is handed (chain 5; nn1_sphere.hpp, SV): the accumulator set that
// iteration's sums launch added into, the state slot, the sums' 19 doubles and — null / 0 where the host wants none — the slot of the host ring and its
// sequence number, all written by workgroup 0 alone; e = the exponent of the accumulation's fixed-point grid (KabschPlan)
struct IcpSolveArgs {
    const long long* acc;
    IcpState* st_out;
    double* out;
    IcpSnapSlot* snap;
    unsigned long long seq;
    int e;
};

// fixed-point grid of one exact Kabsch accumulation (kabsch.hip / numerics.hpp): 2^e bounds every coordinate of a kept pair
struct KabschPlan {
    int e = 0;
    float lim = 0.f;      // 2^e as a float (inf when e >= 128)
    double sc = 0.0;      // 2^(80 - e): coordinates -> two 40-bit limbs
    double sp = 0.0;      // 2^(120 - 2e): products -> three 40-bit limbs
};

struct Comm {
    int nranks = 1;
    int rank = 0;
    void* rccl = nullptr;          // ncclComm_t
    pcr_allreduce_fn cb = nullptr;
    void* cb_user = nullptr;
};

}  // namespace pcr

namespace pcr {
struct Grid; void grid_free(Grid*); struct BtIndex; void bt_free(BtIndex*);
// owners of an index under construction or of a temporary one: release() where ownership passes on (both frees take a partially built object)
struct GridFree { void operator()(Grid* g) const { grid_free(g); } };
struct BtFree { void operator()(BtIndex* b) const { bt_free(b); } };
using GridPtr = std::unique_ptr<Grid, GridFree>;
using BtPtr = std::unique_ptr<BtIndex, BtFree>;
// Handles are told apart by serial numbers, never by address (operator new readily returns the address of the cloud just deleted): a number
// is handed out once per process, so it names one handle, or one state of its content, on every context (api.cpp)
uint64_t next_serial();
}

struct pcr_cloud {
    // id: this handle, for its whole life.  rev: what it holds — cloud_modified takes a fresh one, and with it everything a context remembers
    // about the CONTENT of this cloud (keys[], wpos; pcr_ctx::keys_*) stops matching, whatever context the change went through
    const uint64_t id = pcr::next_serial();
    uint64_t rev = id;
    pcr::Grid* grid = nullptr;   // exact-NN index over this cloud as a target; built lazily, dropped on modification
    pcr::BtIndex* bt = nullptr;  // the matrix-core brute-force filter's operands over this cloud as a target (nn1_brute.hip); same lifetime
    pcr::Grid* knn_grid = nullptr;   // the same index with the wider cell of the last k-NN batch (knn_grid.hip), same lifetime
    double knn_grid_factor = 0.0;    // its cell edge / grid's cell edge
    pcr::Grid* rad_grid = nullptr;   // the index with cell edge 1.01 r of the last radius search (radius_grid.hip), same lifetime
    double rad_grid_r = 0.0;
    float absmax = -1.f;             // largest finite |coordinate| (cloud_absmax), < 0: not computed; same lifetime as the grids
    mutable uint32_t brute_searches = 0;   // exhaustive searches that found no index on this target (the second one builds it); same lifetime
    size_t n = 0;
    size_t cap = 0;     // padded length of each of x, y, z
    float* base = nullptr;   // device; x = base, y = base + cap, z = base + 2*cap
    // a SHARD of a larger cloud (pcr_cloud_shard_spatial): the index every point has in the whole cloud, ascending (device, n entries).
    // "The last kept pair" of an iteration (registration.cpp:939) is then the kept pair with the largest GLOBAL index over all ranks.
    uint32_t* gidx = nullptr;
    // a cloud in the order of a target's index (pcr_cloud_sort_for_target, or the sorted working copy of an ICP loop): orig[t] = the index its
    // point t had before the sort (device, n entries), nullptr for a cloud in its own order.  The caller's clouds own the buffer (orig_buf); a
    // loop's working copy points into ctx->work_orig.  Kept by cloud_modified: a transform keeps the order (tests/test_context_state.py §B)
    uint32_t* orig = nullptr;
    uint32_t* orig_buf = nullptr;
    // which read-back of the context's pinned word 0 counts the target-grid cells this cloud's points occupy (0: none; pcr_ctx::pin_words)
    mutable uint64_t cells_tag = 0;
    float* x() const { return base; }
    float* y() const { return base + cap; }
    float* z() const { return base + 2 * cap; }
};

// a range image resident in HBM (range_image.hip): the cropped f64 image, its labels and, for an image projected from a cloud, the pixel of every point
struct pcr_range_image {
    size_t n_points = 0;         // 0: an image taken from the host (pcr_range_image_from_host_f64)
    int rows = 0, cols = 0;      // the cropped image
    int full_rows = 0, full_cols = 0;
    uint64_t dropped = 0;        // points outside the image or non-finite
    double* image = nullptr;     // rows x cols, -1 = empty
    int32_t* label = nullptr;    // rows x cols, valid while `labelled`
    int32_t* pix = nullptr;      // n_points: r * cols + c in the cropped image, -1 = dropped
    bool labelled = false;
    uint64_t n_labels = 0;
};

struct pcr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    hipDeviceProp_t prop;
    // workspace
    unsigned long long* keys = nullptr;   // (d2_bits << 32 | idx) per query of the last nn1 pass
    size_t keys_cap = 0;
    size_t keys_n = 0;
    // Warm start of the searches inside ICP loops: keys[] still holds correspondences of an earlier search.  Any index < n_tgt
    // is a genuine candidate once re-evaluated exactly against the query, so a stale entry can only make the seed worse, never
    // the result wrong; the bookkeeping below only decides whether the seeds are likely to be GOOD: same source cloud (the
    // previous iteration), or another same-sized source against the same target (the previous ICP run on this pair).
    bool keys_warm = false;               // keys[] was written by a search of an ICP loop
    uint64_t keys_src = 0;                // its source (pcr_cloud::id, 0 = none: identity only — a loop moves its source between searches)
    uint64_t keys_tgt = 0;                // its target (pcr_cloud::id, 0 = none)
    uint64_t keys_src_rev = 0, keys_tgt_rev = 0;   // pcr_cloud::rev of both when keys[] was written: what keys[] is the correspondence OF
    bool keys_caller = false;             // keys[] answers a caller's own search (pcr_nn1_f32_async / _loop), not a search inside another stage
    size_t keys_warm_n = 0;               // number of queries of that search
    // the last move of an ICP loop already turned keys[] into the seeds of the next exhaustive search of (keys_seed_src, keys_seed_tgt):
    // launch_nn1_brute then skips its own seed kernel (consumed by the next search, whatever it is)
    bool keys_seeded = false;
    uint64_t keys_seed_src = 0;           // (pcr_cloud::id)
    uint64_t keys_seed_tgt = 0;
    uint32_t* qperm = nullptr;            // queries grouped by target-grid cell (grid NN)
    size_t qperm_cap = 0;
    size_t qperm_n = 0;
    uint64_t qperm_src = 0;               // (pcr_cloud::id, 0 = nobody's)
    // grid ICP: the working cloud is cell-sorted once (work_orig[t] = original index of its point t), and every search leaves
    // the record position of each winner behind (wpos) for the next warm start and for the Kabsch gather
    uint32_t* wpos = nullptr;
    size_t wpos_cap = 0;
    size_t wpos_n = 0;
    bool wpos_valid = false;
    uint64_t wpos_tgt = 0, wpos_tgt_rev = 0;   // the target whose grid the positions index: (id, rev) — a rebuilt grid has another record order
    uint32_t* work_orig = nullptr;        // (the storage of the working copy's pcr_cloud::orig)
    size_t work_orig_cap = 0;
    // two spare cloud buffers (base, cap): the working copies an ICP call clones and gives back (cloud_release) are re-used by the next
    // clone of the same size instead of two hipMalloc + two hipFree (each free a device synchronisation) per call
    float* spare_base[2] = { nullptr, nullptr };
    size_t spare_cap[2] = { 0, 0 };
    // two counters of the index builds come back through PINNED words behind an event each (a hipMemcpyAsync into pageable memory is ordered only
    // by what the runtime happens to do): [0] the target-grid cells a sorted query cloud occupies (pcr_cloud::cells_tag says whose), [1] the occupied
    // cells of a grid (Grid::occupied_tag says whose).  pin_gen[k] numbers the read-backs of word k; before the next one overwrites it, the value of the
    // last one moves into pin_hist (a ring of the latest PIN_HIST per word), so a later build never takes it from its owner (test_context_state.py §D)
    static constexpr int PIN_HIST = 8;
    uint32_t* pin_words = nullptr;
    hipEvent_t pin_ev[2] = { nullptr, nullptr };
    bool pin_pending[2] = { false, false };
    uint64_t pin_gen[2] = { 0, 0 };
    uint64_t pin_hist_tag[2][PIN_HIST] = {};
    uint32_t pin_hist_val[2][PIN_HIST] = {};
    double* partials = nullptr;           // block rows of the Kabsch pass (8192 x 58 doubles)
    size_t partials_cap = 0;
    double* dev_out = nullptr;            // 128 doubles: reduced sums / limbs + bookkeeping
    double* host_out = nullptr;           // pinned mirror
    void* plane_ws = nullptr;             // plane.hip: [ticket | pad to 256 B][partial counts per workgroup]
    size_t plane_ws_bytes = 0;
    void* scratch = nullptr;              // generic device scratch
    size_t scratch_cap = 0;
    void* host_stage = nullptr;           // pinned staging for uploads / downloads
    size_t host_stage_cap = 0;
    void* coop_host = nullptr;            // small coherent host buffer of the one-wave-per-query k-NN (knn_grid.hip): completion word, results
    uint32_t* coop_ticket = nullptr;      // its wave ticket (device memory)
    uint32_t coop_seq = 0;                // value the completion word takes at the end of the next call
    size_t coop_m = 0;                    // queries of the last call (the ticket counts modulo m)
    uint64_t coop_calls = 0, coop_unseen = 0;   // one-wave calls so far; those whose completion word did not show up in time (pcr_ctx_knn_coop_state)
    void* aux = nullptr;                  // second device scratch (partial results of sliced searches), grows on demand
    size_t aux_cap = 0;
    pcr::IcpState* icp_state_dev = nullptr;    // pipelined ICP: device state, pinned snapshots, snapshot events
    // the grid barrier of the fused sums + move launch (kabsch.hip): ONE monotonic counter in device memory (a line of its own behind the two
    // states, never reset) and the value it has once every workgroup of every launch so far has arrived
    unsigned long long* icp_barrier_dev = nullptr;
    uint64_t icp_barrier_arrived = 0;
    // the accumulators of the sums + solve launch (kabsch.hip icp_sums_solve_kernel): ICP_ACC_SETS sets of ICP_ACC_REPLICAS x ICP_ACC_WORDS
    // int64 behind the counter, zeroed with it; set 0 ALL ZERO between launches of that kernel (the last arriver writes the zeros back), BOTH sets all
    // zero between calls (the chain sums -> search alternates between them).  dirty: a call ended in an error — the next call's first
    // launch clears both
    long long* icp_acc_dev = nullptr;
    bool icp_acc_dirty = false;
    // the pinned, coherent host ring: [0..4) snapshots, [4] upload / final state; its address as the device sees it; the last sequence number handed
    // to a launch that writes a slot itself (never reset); how the last call took its snapshots (pcr_icp_last_snapshots)
    pcr::IcpSnapSlot* icp_state_host = nullptr;
    pcr::IcpSnapSlot* icp_state_host_dev = nullptr;
    unsigned long long icp_snap_seq = 0;
    int icp_last_snapshots = 0;
    hipEvent_t icp_events[4] = { nullptr, nullptr, nullptr, nullptr };
    unsigned long long* grid_stats_dev = nullptr;   // diagnostics of the grid search (tune grid_stats)
    const int* stop_flag_dev = nullptr;        // when set, the correspondence kernels exit early once *flag != 0
    // the chain search -> sums + solve of an ICP loop (icp.cpp).  nn1_move_state: set by the loop around a search that must move its queries
    // by the pending Rd, td of that state first (nn1_sphere.hpp, MV) — the exhaustive dispatcher launches the move-carrying kernel or fails.  nn1_move_l0:
    // the level-0 super-tiles of the last exhaustive search's target if it took the family that has such a form (STRACK3), else 0 — the loop asks after its
    // first search; nn1_moved: the last search WAS that form
    // nn1_solve (with nn1_move_state, chain 5): that search also FINISHES the previous iteration first — nn1_move_state is then that
    // iteration's input state, and the move is by the Rd, td the search works out for itself (nn1_sphere.hpp, SV)
    const pcr::IcpState* nn1_move_state = nullptr;
    const pcr::IcpSolveArgs* nn1_solve = nullptr;
    uint64_t nn1_move_l0 = 0;
    bool nn1_moved = false;
    int icp_last_chain = 0;                    // the tail of the last ICP call's iterations (pcr_icp_last_chain)
    uint64_t loop_iters_hint = 0;              // set by an iterated loop (ICP) for its duration: how many searches of one target may follow (nn1_auto_grid)
    uint32_t* far_list = nullptr;              // far queries handed from the grid walk to the exhaustive kernel: [cap] indices + [1] count
    size_t far_cap = 0;
    pcr::Comm comm;
    std::map<std::string, pcr::ProfEntry> prof;
    int prof_level = 0;                   // 0 off (default: an event pair costs ~6 us of stream time on each side of the kernel),
                                          // 1 correspondence kernels only, 2 every kernel
    std::map<std::string, int64_t> tune;
    // what mfma_verdict (nn1_brute.hip) measured on this device before a matrix-core 1-NN kernel was first chosen: -1 not run yet,
    // 1 = within half of every bound the kernel's analysis assumes, 0 = not (the form is never used on this context)
    int mfma_ok16 = -1, mfma_okbf = -1;
    double mfma_worst16[4] = { 0, 0, 0, 0 }, mfma_worstbf[4] = { 0, 0, 0, 0 };
    double mfma_check_ms = 0.0;           // host wall time the checks took (once per context and form)
    const char* last_nn1_kernel = "";     // family of the last 1-NN launch: htrack / btrack / etrack / ftrack / track / grid
};

namespace pcr {

int fail(pcr_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess);

#define PCR_HIP(ctx, call)                                                   \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return pcr::fail((ctx), PCR_ERR_HIP, #call, e__); \
    } while (0)

int ensure_keys(pcr_ctx* ctx, size_t n);
int ensure_scratch(pcr_ctx* ctx, size_t bytes);
int ensure_stage(pcr_ctx* ctx, size_t bytes);
int ensure_aux(pcr_ctx* ctx, size_t bytes);
// ensure_scratch / ensure_aux for L.bytes(), then L.bind(): every pointer declared on L points into the block
int bind_scratch(pcr_ctx* ctx, const Layout& L);
int bind_aux(pcr_ctx* ctx, const Layout& L);
int64_t tune_get(const pcr_ctx* ctx, const char* key, int64_t dflt);

// profiling: record a (start, stop) event pair around a launch on ctx->stream
struct ProfScope {
    pcr_ctx* ctx;
    const char* name;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(pcr_ctx* c, const char* n, int level = 2);
    ~ProfScope();
};
void prof_flush(pcr_ctx* ctx);

// ---- kernel launchers (defined in the .hip files) --------------------------------------------------
int bt_mfma_selftest(pcr_ctx* ctx, int trials, double worst[4]);
int ht_mfma_selftest(pcr_ctx* ctx, int trials, double worst[4]);
int st_sphere_selftest(pcr_ctx* ctx, int trials, unsigned long long res[4]);   // nn1_brute.hip: the level-1 (chunk sphere) statement of STRACK2
int st_sign_selftest(pcr_ctx* ctx, int trials, unsigned long long res[4]);   // nn1_brute.hip: the sign form's decision, checked on the device
bool mfma_verdict(pcr_ctx* ctx, bool f16);     // cached per context; runs the short self-test on first use
int launch_nn1_brute(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool in_loop);
// keys[i] of the last search <- none where d2 >= gate (the exhaustive kernels are not bounded by a caller's loop gate)
int launch_nn1_gate(pcr_ctx* ctx, size_t ns, float gate);
int launch_nn1_brute_list(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, const uint32_t* qlist, const uint32_t* qcount, uint32_t qcap);
// cap2: the caller only uses neighbours with d2 < cap2 (ICP's max_corres_dist gate) — the walk may stop once no such target can exist
int launch_nn1_grid(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool reuse_perm, float cap2);
// grid radius search with the hw2 contract (radius_grid.hip); *used = false -> the caller runs the exhaustive kernels
struct RadiusRowsDev { uint32_t* rows_dev = nullptr; int32_t* idx_dev = nullptr; double* dist_dev = nullptr; uint64_t total = 0; };
int radius_grid(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* q, double r, double r2max, int64_t* row_ptr_host, int32_t* idx_host, double* dist_host,
                bool* used, RadiusRowsDev* keep = nullptr);
// exact grid k-NN between resident clouds (knn_grid.hip); host outputs idx/val [m x k], found [m] (optional)
int cloud_knn_host(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* q, int k, double cap_s, bool squared, double empty_val, int32_t empty_idx,
                   int32_t* idx, double* val, uint32_t* found);
// the same with the results left on the device: idx / val [m x k], found [m] at the head of a fresh allocation *result (caller frees)
int knn_grid_device(pcr_ctx* ctx, const pcr_cloud* db, const pcr_cloud* q, int k, double cap_s, bool squared, double empty_val, int32_t empty_idx,
                    void** result, int32_t** idx_dev, double** val_dev, uint32_t** found_dev);
// the same for a small batch of host queries (f32 rows): one launch, zero-copy in and out
constexpr size_t KNN_SMALL_MAX = 4096;
int cloud_knn_small(pcr_ctx* ctx, const pcr_cloud* db, const float* q_rows, size_t m, int k, double cap_s, bool squared, double empty_val,
                    int32_t empty_idx, int32_t* idx, double* val);
// device-wide exclusive scan of u32 (grid.hip): totals needs scan_blocks(n) words, grand one word (the sum of all n)
constexpr int SCAN_TILE = 2048;
inline size_t scan_blocks(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
int exclusive_scan_u32(pcr_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n, uint32_t* totals, uint32_t* grand);
// range image (range_image.hip); arguments are validated by the entry points in api.cpp
int ri_create(pcr_ctx* ctx, const pcr_cloud* cloud, double resolution_deg, int width, int height, pcr_range_image** out);
int ri_from_host(pcr_ctx* ctx, const double* image, int rows, int cols, pcr_range_image** out);
int ri_read(pcr_ctx* ctx, const pcr_range_image* img, double* image, int32_t* pixel);
int ri_close(pcr_ctx* ctx, pcr_range_image* img, int pad);
int ri_label(pcr_ctx* ctx, pcr_range_image* img, double phi_deg, double theta_deg, int nn_mode, int32_t* image_label, uint64_t* n_labels);
int ri_assign(pcr_ctx* ctx, const pcr_range_image* img, int32_t* cluster_idx);
int ri_destroy(pcr_ctx* ctx, pcr_range_image* img);
// dispatcher: tune "nn_method" 0 = auto (grid for targets >= 2048 points), 1 = brute force, 2 = grid
// (auto: api.cpp nn1_auto_grid — inside an iterated loop the grid from 128 points on; one-shot searches of a target without an index
// stay exhaustive while queries x targets is small)
bool nn1_auto_grid(const pcr_ctx* ctx, const pcr_cloud* tgt, bool in_loop, size_t ns);
// tells the dispatcher for the duration of a loop how many searches of one target may follow
struct LoopHint {
    pcr_ctx* ctx;
    LoopHint(pcr_ctx* c, uint64_t iters) : ctx(c) { ctx->loop_iters_hint = iters; }
    ~LoopHint() { ctx->loop_iters_hint = 0; }
    LoopHint(const LoopHint&) = delete;
    LoopHint& operator=(const LoopHint&) = delete;
};
int launch_nn1(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, bool reuse_perm, float cap2 = __builtin_inff());
void cloud_modified(pcr_cloud* c);
// What a context remembers about clouds, asked in ONE place each.  Every search writes keys_record; nobody compares an address.
inline void keys_record(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src)
{
    ctx->keys_src = src->id; ctx->keys_src_rev = src->rev;
    ctx->keys_tgt = tgt->id; ctx->keys_tgt_rev = tgt->rev;
    ctx->keys_caller = false;             // (pcr_nn1_f32_async / _loop set it once their search is enqueued)
}
// keys[] is the correspondence of exactly this pair as both clouds are NOW (what pcr_kabsch_sums needs)
inline bool keys_are_of(const pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src)
{
    return ctx->keys_n == src->n && ctx->keys_src == src->id && ctx->keys_src_rev == src->rev && ctx->keys_tgt == tgt->id && ctx->keys_tgt_rev == tgt->rev;
}
// wpos[] indexes the records of the grid tgt has now: written against this target, which was not modified (its grid not rebuilt) since
inline bool wpos_is_of(const pcr_ctx* ctx, const pcr_cloud* tgt, size_t ns)
{
    return ctx->wpos_valid && ctx->wpos && ctx->wpos_n == ns && ctx->wpos_tgt == tgt->id && ctx->wpos_tgt_rev == tgt->rev && tgt->grid != nullptr;
}
// gives a cloud back WITHOUT synchronising the stream: its buffer goes to the context's spare slots (or is freed when both are taken).
// Safe for work enqueued on ctx->stream that still reads the cloud: the buffer stays allocated, and whoever gets it next writes it on
// the same stream.  (pcr_cloud_destroy = the same behind a stream synchronisation: the public contract.)
void cloud_release(pcr_ctx* ctx, pcr_cloud* c);
int grid_sort_working_cloud(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud** work, bool in_place = false);
int bt_sort_working_cloud(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud** work, bool in_place = false);
int nn1_unpack(pcr_ctx* ctx, size_t n, uint32_t* idx_dev, float* d2_dev);
int cloud_shard_spatial(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* full, int nranks, int rank, int chunks_per_rank, pcr_cloud** out,
                        int (*alloc)(pcr_ctx*, size_t, pcr_cloud**));
int launch_transform(pcr_ctx* ctx, pcr_cloud* c, const float R[9], const float t[3]);
// dst (a fresh allocation of src's size: cloud_alloc) = R src + t, padding included — the clone and the transform of a loop's working copy in one launch
int launch_transform_into(pcr_ctx* ctx, const pcr_cloud* src, pcr_cloud* dst, const float R[9], const float t[3]);
int cloud_alloc(pcr_ctx* ctx, size_t n, pcr_cloud** out);     // api.cpp: an uninitialised cloud of n points (from the parked buffers when one fits)
int cloud_absmax(pcr_ctx* ctx, const pcr_cloud* c, float* out);       // largest finite |coordinate|, cached on the cloud (grid.hip)
int kabsch_grid_exponent(float target_absmax, float max_corr);
int kabsch_plan(pcr_ctx* ctx, const pcr_cloud* tgt, float max_corr, KabschPlan* plan);
// dev_out[0..18] = the 16 moments, original index of the last kept pair (or -1), its d2, overflow flag
int launch_kabsch_sums(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr, const KabschPlan& plan);
int launch_kabsch_partial(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* src, float max_corr, const KabschPlan& plan, uint32_t* n_blocks);
int launch_icp_update(pcr_ctx* ctx, uint32_t n_blocks, IcpState* st_dev, const KabschPlan& plan);
// dev_out[0..54] limbs, [55] overflow flag, [56 + 2r], [57 + 2r] (order key of the last kept pair — 0 = none kept —, its d2) of rank r:
// ICP_NRED(nranks) doubles to all-reduce; gidx: the shard's global indices (key = global index + 1), or nullptr (key = rank + 1: contiguous shards in rank order)
int launch_icp_reduce_slots(pcr_ctx* ctx, uint32_t n_blocks, int nranks, int rank, bool have_points, const uint32_t* gidx = nullptr);
int launch_icp_update_from_sums(pcr_ctx* ctx, int nranks, IcpState* st_dev, const KabschPlan& plan);
inline int icp_nred(int nranks) { return 56 + 2 * nranks; }
// seed_tgt != nullptr: the move also writes the seeds of the next exhaustive search into keys[] (kabsch.hip seed_next_search)
int launch_transform_state(pcr_ctx* ctx, pcr_cloud* c, IcpState* st_dev, const pcr_cloud* seed_tgt = nullptr);
// small clouds, one rank: icp_update + transform_state in one launch; the state alternates between the two buffers st_in / st_out
int launch_icp_update_move(pcr_ctx* ctx, uint32_t n_blocks, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan, pcr_cloud* c,
                           const pcr_cloud* seed_tgt = nullptr);
// exhaustive loops, one rank, a grid of at most one workgroup per CU: kabsch_partial + icp_update_move in ONE launch whose workgroups meet once at a
// grid barrier.  icp_fused_sums_blocks = the workgroups it would take (0: the cloud or the device rules it out)
uint32_t icp_fused_sums_blocks(const pcr_ctx* ctx, size_t n);
int launch_icp_sums_update_move(pcr_ctx* ctx, const pcr_cloud* tgt, pcr_cloud* c, float max_corr, const IcpState* st_in, IcpState* st_out,
                                const KabschPlan& plan, const pcr_cloud* seed_tgt);
// the chain search (moves the cloud by the previous solve) -> sums + solve: the front half of the launch above and a ticket, the last
// workgroup to arrive reduces and solves; nobody waits and nothing moves.  A workgroup's totals go out as int64 atomic adds into ctx->icp_acc_dev, not
// as a row.  icp_sums_solve_blocks = its workgroups (0: switched off, too few points, or 2^22 points and more).  snap: null, or the slot
// of the host ring (device address) the publishing workgroup also writes the state to, followed by a system-scope release store of seq
uint32_t icp_sums_solve_blocks(const pcr_ctx* ctx, size_t n);
int launch_icp_sums_solve(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* c, float max_corr, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan,
                          IcpSnapSlot* snap, unsigned long long seq);
// chain 5: the sums alone into accumulator set `set` (and zeros over the other one); the reduce and the solve are the next search's
// (ctx->nn1_solve) or, behind the last iteration of a call, launch_icp_finish's: one wave that publishes like the sums + solve launch and zeroes its set
int launch_icp_sums(pcr_ctx* ctx, const pcr_cloud* tgt, const pcr_cloud* c, float max_corr, const IcpState* st_in, const KabschPlan& plan, int set);
int launch_icp_finish(pcr_ctx* ctx, const IcpState* st_in, IcpState* st_out, const KabschPlan& plan, int set, IcpSnapSlot* snap, unsigned long long seq);
// nn1_brute.hip: can a seeded STRACK3 search of ns queries over n_l0 level-0 super-tiles carry the move (transposed form, one slice)?  Raw tune values
uint64_t s3_l0_super_tiles(uint64_t n_tgt);          // the level-0 super-tiles the index of a target of n_tgt points has (bt_ensure_l1)
bool s3_move_route(uint64_t n_l0, uint64_t ns, int64_t transposed_tune, int64_t qg_tune, int64_t l0_per_slice_tune, int64_t blocks_tune);
// icp.cpp: the loop's own conditions for that chain, from plain numbers (pcr_icp_move_route)
bool icp_move_route(uint64_t n_src, uint64_t n_l0, int nranks, int64_t move_in_search_tune, int64_t fused_sums_tune, int64_t fused_sums_min_tune,
                    int64_t transposed_tune, int64_t qg_tune, int64_t l0_per_slice_tune, int64_t blocks_tune);
// ... and, where that chain would be taken, whether the solve moves into the next search as well (chain 5; pcr_icp_solve_route): raw values of the
// tunes icp_solve_in_search and icp_move_in_search; auto is bounded by the source size
bool icp_solve_route(uint64_t n_src, int64_t solve_in_search_tune, int64_t move_in_search_tune);
int comm_allreduce_f64_device(pcr_ctx* ctx, double* dev_buf, int n);   // RCCL on the ctx stream, no host round trip
int launch_plane_count(pcr_ctx* ctx, const pcr_cloud* pts, const double* planes4_host, size_t n_planes,
                       double thr, unsigned long long* counts_out);
int launch_plane_mask(pcr_ctx* ctx, const pcr_cloud* pts, const double plane4[4], double thr,
                      uint8_t* mask_dev, unsigned long long* count_dev);
int launch_knn_f64(pcr_ctx* ctx, const double* db_soa, size_t n, size_t n_cap, const double* q_soa, size_t m,
                   int k, int32_t* idx_dev, double* dist_dev, bool squared);
int launch_radius_count(pcr_ctx* ctx, const double* db_soa, size_t n, size_t n_cap, const double* q_soa,
                        size_t m, double r, unsigned long long* counts_dev, uint32_t slices);
int launch_radius_fill(pcr_ctx* ctx, const double* db_soa, size_t n, size_t n_cap, const double* q_soa,
                       size_t m, double r, const long long* row_ptr_dev, int32_t* idx_dev, double* dist_dev, uint32_t slices);

// ---- PointNet++ sampling on device buffers (pointnet.hip), for callers that chain stages without a host round trip (pointnet2.hip) --------
// one FPS segment: points [base, base + n) of the coordinate arrays, first pick (segment-local), row of the output
struct FpsJob {
    uint32_t base, n, start, out_row;
};
// host arrays an asynchronous upload still reads: the caller keeps them until it has synchronised the stream
struct HostKeep {
    std::vector<std::shared_ptr<void>> held;
};
// the picks of every job into out_dev[job.out_row][npoint]; enqueues on ctx->stream and does NOT synchronise (the job tables live in `keep`).
// Same kernels and the same rule as pcr_fps_f32.  Uses ctx->aux.
int fps_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, std::vector<FpsJob> jobs, uint32_t npoint, int mode, uint32_t* out_dev, HostKeep* keep);
// pcr_ball_query_f32's kernel on device tables: seg_dev[n_seg + 1], centre_seg_dev[nq] (the segment of every centre), idx_dev[nq][nsample], cnt_dev[nq]
int ball_query_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, const float* qx, const float* qy, const float* qz, const uint32_t* seg_dev,
                      const uint32_t* centre_seg_dev, size_t nq, double radius, size_t nsample, uint32_t* idx_dev, uint32_t* cnt_dev);
// pcr_ball_query_multi_f32's kernel on device tables: n_radii in 1 ... 4; per radius b idx_dev[b][nq][nsamples[b]] and cnt_dev[b][nq]
int ball_query_multi_device(pcr_ctx* ctx, const float* x, const float* y, const float* z, const float* qx, const float* qy, const float* qz, const uint32_t* seg_dev,
                            const uint32_t* centre_seg_dev, size_t nq, size_t n_radii, const double* radii, const uint32_t* nsamples, uint32_t* const* idx_dev,
                            uint32_t* const* cnt_dev);
// SplitMix64 keying of include/pcr.h: K(seed, a)
inline unsigned long long splitmix_key(unsigned long long seed, unsigned long long a)
{
    unsigned long long zz = seed ^ (0x9E3779B97F4A7C15ull * (a + 1ull));
    zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
    zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
    return zz ^ (zz >> 31);
}

// ---- host numerics ------------------------------------------------------------------------------------
void svd3(const double A[9], double U[9], double S[3], double V[9]);
int kabsch_solve(const double sums[16], float R[9], float t[3]);
// the same solve in its lane form (kabsch_wave.hpp): by the host's lane group, and by one wave per problem on the device (kabsch.hip; host arrays in and out)
int kabsch_solve_lanes(const double sums[16], float R[9], float t[3]);
int kabsch_solve_batch_device(pcr_ctx* ctx, const double* sums, size_t n, float* R, float* t, int* rc);
void mat4_mul_f32(const float A[16], const float B[16], float out[16]);
// every eigenpair of a real n x n matrix, n <= 16 (numerics.cpp; the contract of pcr_eig_small_f64), and the eigengap rule of Homework3
int eig_small(int n, const double* a, double* wr, double* wi, double* vec);
// the same for n <= 32, after the permutation that isolates eigenvalues (a row or column with zeros off the diagonal): the dense path of spectral.hip
int eig_dense(int n, const double* a, double* wr, double* wi, double* vec);
int spectral_select_k(const double* eig, int n_eig);
// the device rows of a pcr_mat64 (mixture.hip owns the struct): row-major n x dim
const double* mat64_rows_dev(const pcr_mat64* m);

// ---- collectives ----------------------------------------------------------------------------------------
int comm_allreduce_f64(pcr_ctx* ctx, double* host_buf, double* dev_buf, int n);
// the slot of the globally last kept pair in a summed reduce row (the largest order key), or -1: the same rule on host and device
__host__ __device__ inline int icp_last_slot(const double* buf, int nranks)
{
    int best = -1;
    double key = 0.5;
    for (int r = 0; r < nranks; r++)
        if (buf[56 + 2 * r] > key) { key = buf[56 + 2 * r]; best = r; }
    return best;
}

}  // namespace pcr
