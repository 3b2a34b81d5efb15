// pt_context.hip -- host side of the C-ABI (include/pt_abi.h): persistent device context, scene/camera
// flattening, launch sequencing, hipGraph capture, event timing.
//
// Replaces the host body of cudaRaytraceCore (ref: src/raytraceKernel.cu:106-165): instead of
// cudaMalloc + H2D + 2 launches + D2H + cudaFree on every iteration, the context keeps the framebuffer,
// ray pools and scene resident and enqueues 1 + depth launches per iteration with no host round trip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_internal.h"
#include "pt_scene.h"
#include "pt_tables.h"

// library choices of the resident-path launch (pt_options.resident == 0; measurements in DESIGN.md section 5.1)
#ifndef PT_RESIDENT_DEFAULT
#define PT_RESIDENT_DEFAULT 1
#endif
#ifndef PT_REFILL_MIN_DEFAULT
#define PT_REFILL_MIN_DEFAULT 8
#endif

namespace {
thread_local std::string g_last_error;
}

int pt::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

namespace {

using pt::fail;
using pt::lerp3;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(PT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

#define PT_TRY(expr)                                                                                   \
    do {                                                                                               \
        const int rc__ = (expr);                                                                       \
        if (rc__ != PT_OK) return rc__;                                                                \
    } while (0)

}  // namespace

struct pt_ctx {
    int device = 0;
    int cu_count = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    pt_options opt;
    bool have_scene = false, have_camera = false;
    std::vector<pt_static_geom> geoms;
    std::vector<pt_material> mats;
    pt_camera_data cam;
    // triangles of the MESH geoms (pt_set_meshes), object space: 9 floats each + the geom they belong to
    std::vector<float> tri_obj;
    std::vector<int> tri_geom;
    // motion blur (pt_set_motion): one child context per shutter slice, all rendering into THIS context's framebuffer
    // on this context's stream; pt_render hands every run of 16 iterations to the slice it belongs to
    std::vector<pt_static_geom> geoms_next;
    pt_camera_data cam_next;
    bool have_cam_next = false;
    int motion_slices = 0, motion_rotat = 0;
    std::vector<pt_ctx *> slice_ctx;
    bool motion_dirty = false;

    // device state
    bool dirty = true;          // scene / camera / options changed since the last configure
    pt::KParams kp;             // sequence 0's parameters (what everything outside the launch sequencing reads)
    pt::KParams kps[PT_MAX_SEQUENCES];   // per launch sequence: own ray pools, radiance planes and IterState
    int nseq = 1;               // launch sequences in flight (pt_options.sequences)
    hipStream_t seq_stream[PT_MAX_SEQUENCES] = {};   // [0] = `stream`; [k > 0] own streams
    hipEvent_t seq_acc[PT_MAX_SEQUENCES] = {};       // recorded behind a sequence's accumulate
    hipEvent_t seq_fork = nullptr;
    pt::LaunchCfg cfg;
    ptd::Prim *d_prims = nullptr;
    float *d_mats = nullptr;
    float *d_ro_eye = nullptr;
    float *d_face_n = nullptr;
    float *d_box_eye = nullptr;
    uint32_t *d_span_off = nullptr, *d_span_list = nullptr;
    size_t span_off_cap = 0, span_list_cap = 0;
    uint32_t *d_span_mask = nullptr;
    size_t span_mask_cap = 0;
    float *d_box_world = nullptr;
    float *d_slab_n = nullptr;          // per primitive (n.xyz, d_lo) of the pre-test's slab (KParams::slab_mask)
    pt::LightRec *d_lights = nullptr;    // direct lighting: the light table
    float *d_knots = nullptr, *d_knot_cam = nullptr;   // per-ray motion blur: knot states (matrices, camera vectors)
    int *d_light_tris = nullptr;         //   mesh lights: triangle numbers ...
    float *d_light_cdf = nullptr;        //   ... and the running sums of their areas
    ptd::BvhNode *d_bvh = nullptr;
    float *d_bvh4 = nullptr;    // 4-wide hierarchy (geom_path 7)
    float *d_image_own = nullptr;
    float *d_image_bound = nullptr;
    size_t image_bytes = 0, image_cap = 0;
    void *d_pool = nullptr;
    size_t pool_cap = 0;
    float *d_lbuf = nullptr;    // per-iteration radiance planes of the running batch
    size_t lbuf_cap = 0;
    unsigned long long batches_stamped = 0;   // batches rendered since the radiance planes were last zeroed (serial-number budget)
    int batch = 1;              // iterations in flight per launch sequence
    pt::IterState *d_state = nullptr;          // PT_MAX_SEQUENCES of them
    bool image_valid = false;   // framebuffer holds iterations 1..k of the current frame

    // one batch of one sequence (bookkeeping, depth bounce launches; with a single sequence also the accumulate); the
    // batch's iteration count lives on the device, so this graph serves every pt_render
    // slots [0, PT_MAX_SEQUENCES): a sequence's batch without the accumulate; slot PT_MAX_SEQUENCES: sequence 0's with it
    hipGraph_t graph[PT_MAX_SEQUENCES + 1] = {};
    hipGraphExec_t graph_exec[PT_MAX_SEQUENCES + 1] = {};

    std::vector<std::pair<hipEvent_t, hipEvent_t>> timers;
    double gpu_ms = 0.0;
    unsigned long long bounce_launches = 0;
};

namespace {

void drop_graph(pt_ctx *c)
{
    for (int q = 0; q <= PT_MAX_SEQUENCES; ++q) {
        if (c->graph_exec[q]) { (void)hipGraphExecDestroy(c->graph_exec[q]); c->graph_exec[q] = nullptr; }
        if (c->graph[q]) { (void)hipGraphDestroy(c->graph[q]); c->graph[q] = nullptr; }
    }
}

// Every stream the context may have work on: the render stream and the side streams of the launch sequences.  Whoever needs the
// context idle (configure, statistics, image copies, the error paths of pt_render after its fork) waits for all of them, so a
// call that failed between fork and join cannot leave a side stream running against buffers the next call reuses.
hipError_t sync_all_streams(pt_ctx *c)
{
    hipError_t first = hipStreamSynchronize(c->stream);
    for (int sq = 1; sq < PT_MAX_SEQUENCES; ++sq)
        if (c->seq_stream[sq]) {
            const hipError_t e = hipStreamSynchronize(c->seq_stream[sq]);
            if (first == hipSuccess) first = e;
        }
    return first;
}

int fold_timers(pt_ctx *c)
{
    for (auto &t : c->timers) {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(t.second));
        HIP_TRY(hipEventElapsedTime(&ms, t.first, t.second));
        c->gpu_ms += (double)ms;
        (void)hipEventDestroy(t.first);
        (void)hipEventDestroy(t.second);
    }
    c->timers.clear();
    return PT_OK;
}

float *image_ptr(pt_ctx *c) { return c->d_image_bound ? c->d_image_bound : c->d_image_own; }

// motion blur modes: one scene state per run of 16 iterations (child contexts), or a shutter time per ray
bool motion_by_slices(const pt_ctx *c) { return c->motion_slices > 1 && !c->opt.motion_per_ray && !c->geoms_next.empty(); }
bool motion_per_ray(const pt_ctx *c) { return c->motion_slices >= 1 && c->opt.motion_per_ray && !c->geoms_next.empty(); }

// a scene table to the device (d) and into the kernels' parameters (kp): the old copy goes, the new one has at least one element
template <class T>
int upload(T *&d, const std::vector<T> &v, const T *&kp)
{
    if (d) { (void)hipFree(d); d = nullptr; }
    HIP_TRY(hipMalloc((void **)&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    kp = d;
    return PT_OK;
}

// a camera-ray span table of n entries: its buffer only ever grows
int reserve(uint32_t *&d, size_t &cap, size_t n)
{
    if (cap >= n) return PT_OK;
    if (d) (void)hipFree(d);
    d = nullptr; cap = 0;
    HIP_TRY(hipMalloc((void **)&d, n * sizeof(uint32_t)));
    cap = n;
    return PT_OK;
}

// launch shape for the scene in `k`: persistent workgroups, as many as are resident at once (c->cfg, c->batch, c->nseq; k.cull, nshard,
// refill_min, nslot, slab_mask)
int choose_launch(pt_ctx *c, pt::KParams &k)
{
    const pt_options &o = c->opt;
    const int npix = k.npix;
    pt::LaunchCfg &cfg = c->cfg;
    cfg.workgroup = o.workgroup ? o.workgroup : 256;
    // library choice: the pair queue's pre-test is linear in the primitive count, the hierarchy walks logarithmic:
    // measured crossover near 40 primitives (profiles/r01/crossover_pair_vs_walk.txt); above it the batched 4-wide walk
    cfg.geom = o.geom_path == 0 ? (k.nG <= 40 ? 4 : 6) : o.geom_path - 1;
    if (k.ntri > 0) {
        // triangle records are understood by the scalar loop and the batched walks only
        if (o.geom_path == 0) cfg.geom = 6;
        else if (!(cfg.geom == 0 || cfg.geom == 6 || cfg.geom == 7))
            return fail(PT_ERR_INVALID, "scenes with triangle meshes need geom_path 0, 1, 7 or 8 (got %d)", o.geom_path);
    }
    // the batched walks and the pair queues keep 20-bit primitive / node indices beside their flag bits
    if ((cfg.geom == 4 || cfg.geom == 5 || cfg.geom == 6 || cfg.geom == 7) && (k.nG >= (1 << 20) || k.nnodes4 >= (1 << 20))) {
        if (o.geom_path != 0)
            return fail(PT_ERR_INVALID, "%d primitives (triangles included), %d wide nodes: at most %d on this geometry path", k.nG, k.nnodes4, (1 << 20) - 1);
        cfg.geom = 0;
    }
    // the batched walk's entry ring must hold a full batch above its depth-first reserve (pt_bounce.h W4_STACK = 512): a
    // degenerate hierarchy (e.g. sizes in a long geometric progression) can be deeper than that allows
    if ((cfg.geom == 6 || cfg.geom == 7) && 64 + 3 * k.wdepth + 4 > 512) {
        if (o.geom_path != 0)
            return fail(PT_ERR_INVALID, "hierarchy depth %d: the batched walk's entry ring holds at most depth %d", k.wdepth, (512 - 64 - 4) / 3);
        cfg.geom = 0;
    }
    cfg.compact = o.compaction;
    cfg.nee = k.nlights > 0 ? 1 : 0;             // no lights: nothing to sample, the plain kernels are exact
    // the scattering kernels only when some material that can hold a medium asks for it: else the plain kernels are exact
    cfg.motion = k.nknots > 0 ? 1 : 0;
    // (per-ray shutter time: the pair queue up to 40 primitives -- pre-test against the swept boxes, exact tests in full batches with
    // per-pair interpolated rows --, the scalar loop above that or on request)
    if (cfg.motion) { cfg.geom = (o.geom_path == 5 || (o.geom_path == 0 && k.nG <= 40)) ? 4 : 0; cfg.workgroup = 256; }
    cfg.media = 0;
    if (k.scatter)
        for (const pt_material &m : c->mats)
            if (m.hasScatter > 0.0f && !(m.hasReflective > 0.0f)) cfg.media = 1;
    if (cfg.media && !(cfg.workgroup == 256 || cfg.workgroup == 512))
        return fail(PT_ERR_INVALID, "scatter needs workgroup 0, 256 or 512 (got %d)", cfg.workgroup);
    k.cull = (k.nG > 32 && !getenv("PT_NO_CULL")) ? 1 : 0;
    k.nshard = (cfg.compact == 1) ? pt::NSHARD : 1;
    // the pre-test with slabs (pair path): kernel instances of their own, taken only where a cube of the scene has a slab (decided again at
    // the end, should a fallback below change the launch shape)
    auto slab_wanted = [&]() {
        return (k.slab_mask != 0u && cfg.geom == 4 && cfg.compact == 1 && (cfg.workgroup == 256 || cfg.workgroup == 512) && !cfg.nee && !cfg.media &&
                !cfg.motion) ? 1 : 0;
    };
    cfg.slab = slab_wanted();
    // resident paths (pt_options.resident): the camera launch as ever, then ONE launch that traces bounces 1 .. depth - 1 with the
    // paths kept in registers -- where a kernel instance exists (pair queue / batched walks, plain kernels) and there is more
    // than one later bounce to fuse; everything else keeps the launch per bounce
    {
        int want = o.resident;
        if (want == 0 && getenv("PT_RESIDENT")) want = atoi(getenv("PT_RESIDENT")) > 0 ? 1 : -1;      // (only when the option leaves the choice open)
        // Library choice: from 5 bounces on.  The one launch saves depth - 2 launches and their tails and pays with a drain (the last
        // paths of every wave run up to depth - 1 trips alone): 1920x1080: - 5 % / +- 0 / + 4 % / + 4 % at depth 3 / 4 / 5 / 6;
        // 400x400: - 13 % / - 4 % / + 1 % / + 3 % (profiles/r04/ab_resident_paths.txt).  An explicit 1 takes it from 3 bounces on.
        // With direct lighting or scattering the instances exist and are bit-exact, but do not pay (config 2 with direct lighting - 3.4 %,
        // configs 3 / 5 +- 0 / + 1 %: the shadow-ray pass doubles a trip's work and halves the drain's weight): on request only.
        const int min_depth = (want == 0) ? 5 : 3;
        if (want == 0) want = (cfg.nee || cfg.media) ? -1 : PT_RESIDENT_DEFAULT;
        cfg.resident = 0;
        if (want > 0 && k.depth >= min_depth) {
            pt::LaunchCfg t = cfg;
            if ((t.geom == 6 || t.geom == 7) && o.workgroup == 0) t.workgroup = 512;     // (the walks pick 256 or 512 below: both exist)
            cfg.resident = pt::bounce_resident_available(t) ? 1 : 0;
        }
        k.refill_min = getenv("PT_REFILL_MIN") ? atoi(getenv("PT_REFILL_MIN")) : PT_REFILL_MIN_DEFAULT;
        if (k.refill_min < 1) k.refill_min = 1;
        if (k.refill_min > 64) k.refill_min = 64;
    }
    size_t lds = pt::bounce_lds_bytes(k, cfg);
    if ((cfg.geom == 6 || cfg.geom == 7) && o.workgroup == 0) {
        // the batched walk keeps 4.5 KiB of LDS per wave beside the node copy: take the workgroup size that puts most
        // waves on a CU (a larger workgroup shares one node copy among more waves)
        int best_wg = cfg.workgroup;
        long long best_waves = 0;
        for (int wg : {256, 512}) {
            pt::LaunchCfg t = cfg;
            t.workgroup = wg;
            const long long fit = (160LL * 1024) / ((long long)pt::bounce_lds_bytes(k, t) + 1300);
            const long long waves = std::min<long long>(fit * (wg / 64), 24);
            if (waves > best_waves) { best_waves = waves; best_wg = wg; }
        }
        cfg.workgroup = best_wg;
        lds = pt::bounce_lds_bytes(k, cfg);
    }
    if (cfg.geom == 6 && lds > 96 * 1024 && o.geom_path == 0) {
        cfg.geom = 7;                              // node copy too large for the LDS: the same walk, nodes through L1/L2
        cfg.workgroup = o.workgroup ? o.workgroup : 256;
        lds = pt::bounce_lds_bytes(k, cfg);
    }
    if (lds > 160 * 1024 && o.geom_path == 0) {
        // the hierarchy (32 B per node, 2 nodes per primitive) no longer fits the CU's LDS: fall back to the scalar
        // loop with the per-wave bounding-sphere cull, which needs none
        cfg.geom = 0;
        lds = pt::bounce_lds_bytes(k, cfg);
    }
    if (lds > 160 * 1024) return fail(PT_ERR_INVALID, "scene needs %zu B of LDS per workgroup (> 160 KiB)", lds);
    int per_cu = pt::bounce_max_blocks_per_cu(k, cfg);
    if (per_cu < 1) return fail(PT_ERR_HIP, "occupancy query failed for workgroup=%d (%s)", cfg.workgroup,
                                hipGetErrorString(hipGetLastError()));
    // The occupancy query over-counts near the LDS limit: 5 workgroups of 31.2 KB are resident together, 5 of 31.8 KB are
    // not (measured), i.e. about 1.3 KB per workgroup is spoken for.  A persistent grid sized for workgroups that are not
    // resident runs them as a second round (-7...-23 %), so the count is corrected here.
    {
        const long long fit = (160LL * 1024) / ((long long)lds + 1300);
        if (fit >= 1 && per_cu > (int)fit) per_cu = (int)fit;
    }
    // Persistent grid: 6 workgroups of 256 threads per CU is the measured optimum (config 2: 4 -> 32.0, 5 -> 34.0,
    // 6 -> 34.5, 7 -> 30.5 G ray-bounces/s; the same shape on the glass scene and at 4K): a seventh costs 11 %.
    int cap = 6 * 256 / cfg.workgroup;
    if (cap < 1) cap = 1;
    if (getenv("PT_MAX_WG_PER_CU") && atoi(getenv("PT_MAX_WG_PER_CU")) > 0) cap = atoi(getenv("PT_MAX_WG_PER_CU"));
    if (per_cu > cap) per_cu = cap;
    // iterations in flight per launch sequence: every bounce launch then carries batch x npix paths, which
    // amortises the per-launch fixed cost (launch, LDS staging, ramp, tail) over `batch` samples per pixel
    int batch = o.batch == 0 ? pt::PT_MAX_BATCH : o.batch;
    while (batch > 1 && (long long)npix * batch > (1LL << 28)) --batch;
    if (npix >= (1 << 27)) return fail(PT_ERR_INVALID, "tile of %d pixels too large (pixel index must fit 27 bits)", npix);
    c->batch = batch;
    k.nslot = batch;
    const long long nrays = (long long)npix * batch;
    const long long want = (nrays + cfg.workgroup - 1) / cfg.workgroup;
    long long grid = (long long)c->cu_count * per_cu;
    if (grid > want) grid = want;
    if (grid < 1) grid = 1;
    cfg.grid = (int)grid;
    if (cfg.resident && !pt::bounce_resident_available(cfg)) cfg.resident = 0;      // (a fallback above changed the launch shape)
    cfg.slab = slab_wanted();
    if (!cfg.slab) k.slab_mask = 0u;
    if (getenv("PT_DEBUG_CLOCK"))
        fprintf(stderr, "[ptamd] launch: geom %d, workgroup %d, %zu B LDS, %d workgroups/CU, grid %d, batch %d, resident paths %d (refill at %d free lanes)\n", cfg.geom, cfg.workgroup,
                lds, per_cu, cfg.grid, batch, cfg.resident, k.refill_min);

    // Launch sequences in flight: sequence q renders batches q, q + nseq, ... of a pt_render call on a stream of its own,
    // with its own ray pools, radiance planes and IterState; only the accumulates are ordered across the sequences
    // (iteration order).  The workgroups of a bounce launch do not finish together -- their lifetimes spread over
    // 65..100 % of the launch -- and a second sequence's launches fill the compute units the first one's tail leaves idle.
    // Library choice: two (config 2 on one box: 37.2 / 43.0 / 42.9 / 41.4 G ray-bounces/s with 1 / 2 / 3 / 4 sequences;
    // config 5: 17.7 / 20.5 / 19.7 / 18.8 G -- profiles/r03/sweep_sequences.txt).
    int nseq = o.sequences == 0 ? 2 : o.sequences;
    // (the environment only where the option leaves the choice to the library; pt_get_launch_info reports what was taken)
    if (o.sequences == 0 && getenv("PT_SEQUENCES") && atoi(getenv("PT_SEQUENCES")) >= 1 && atoi(getenv("PT_SEQUENCES")) <= PT_MAX_SEQUENCES)
        nseq = atoi(getenv("PT_SEQUENCES"));
    c->nseq = nseq;
    return PT_OK;
}

// the scene tables to the device, in k's pointers
int upload_tables(pt_ctx *c, const pt::SceneTables &t, pt::KParams &k)
{
    PT_TRY(upload(c->d_lights, t.lights, k.lights));
    PT_TRY(upload(c->d_light_tris, t.light_tris, k.light_tris));
    PT_TRY(upload(c->d_light_cdf, t.light_cdf, k.light_cdf));
    PT_TRY(upload(c->d_prims, t.prims, k.prims));
    PT_TRY(upload(c->d_ro_eye, t.ro_eye, k.ro_eye));
    PT_TRY(upload(c->d_face_n, t.face_n, k.face_n));
    PT_TRY(upload(c->d_slab_n, t.slab_n, k.slab_n));
    PT_TRY(upload(c->d_box_eye, t.box_eye, k.box_eye));
    PT_TRY(upload(c->d_box_world, t.box_world, k.box_world));
    PT_TRY(upload(c->d_mats, t.mat_planes, k.mats));
    if (k.nknots > 0) {
        PT_TRY(upload(c->d_knots, t.knots, k.knots));
        PT_TRY(upload(c->d_knot_cam, t.knot_cam, k.knot_cam));
        // (the pair path's pre-test of a moving primitive: its box swept over the shutter interval)
        if (!t.swept.empty()) HIP_TRY(hipMemcpy(c->d_box_world, t.swept.data(), t.swept.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    PT_TRY(upload(c->d_bvh4, t.bvh4, k.bvh4));
    PT_TRY(upload(c->d_bvh, t.bvh, k.bvh));
    return PT_OK;
}

// camera-ray span tables of the chosen launch shape (pt_tables.h), if it takes any
int upload_spans(pt_ctx *c, const pt::SceneTables &t, pt::KParams &k)
{
    const std::vector<uint32_t> tab = pt::span_mask(k, c->cfg, t);
    if (!tab.empty()) {
        PT_TRY(reserve(c->d_span_mask, c->span_mask_cap, tab.size()));
        HIP_TRY(hipStreamSynchronize(c->stream));          // (launches of the previous configuration may still read the table)
        HIP_TRY(hipMemcpy(c->d_span_mask, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        k.span_mask = c->d_span_mask;
    }
    std::vector<uint32_t> off, lst;
    pt::span_lists(k, c->cfg, t, off, lst);
    if (!off.empty()) {
        PT_TRY(reserve(c->d_span_off, c->span_off_cap, off.size()));
        PT_TRY(reserve(c->d_span_list, c->span_list_cap, lst.size()));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(c->d_span_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_span_list, lst.data(), lst.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        k.span_off = c->d_span_off;
        k.span_list = c->d_span_list;
    }
    return PT_OK;
}

// ray pools and radiance planes of the launch sequences, then every sequence's KParams (k: sequence 0's)
int allocate_sequences(pt_ctx *c, pt::KParams &k)
{
    int nseq = c->nseq;
    const long long nrays = (long long)k.npix * c->batch;
    const pt::LaunchCfg &cfg = c->cfg;
    // per-iteration radiance planes (one write per path, folded into the image by k_accumulate), per sequence
    // (16-byte entries: r, g, b and the serial number of the batch that wrote them; zeroed once -- no batch has serial 0)
    const size_t lbuf_bytes = ((size_t)nrays * 4 * sizeof(float) + 255) & ~(size_t)255;
    // ray pools: 2 x nshard segments of `segcap` rays x 40 B, carved from one allocation.  A segment must hold
    // every survivor its writers can produce in one launch: each wave appends at most 64 rays per round and runs
    // at most `rounds` rounds (chunks are 64 rays; per-segment padding adds at most NSHARD chunks).
    {
        const long long nw = cfg.workgroup / 64;
        const long long total_waves = (long long)cfg.grid * nw;
        const long long chunks = (nrays + 63) / 64 + pt::NSHARD;
        const long long rounds = (chunks + total_waves - 1) / total_waves;
        long long writers = total_waves;                                   // nshard == 1: everyone writes segment 0
        if (k.nshard > 1) writers = (total_waves + k.nshard - 1) / k.nshard;
        long long segcap = writers * rounds * 64;
        const long long npad = (nrays + 63) & ~63LL;
        if (k.nshard == 1 || segcap > npad) segcap = npad;                 // never more than all rays
        k.segcap = (uint32_t)segcap;
    }
    const size_t slots = (size_t)k.segcap * (size_t)k.nshard;
    const size_t one = slots * (16 + 16 + 8);
    // Device memory per launch sequence: two ray pools of 40 B per slot (<= 1.16 x batch x pixels slots) and the radiance planes,
    // 16 B per (iteration in flight, pixel) -- 6.5 GB per sequence for a 1920x1080 tile at batch 16, ~ 52 GB at the 2^28-ray cap.
    // When the allocation for the sequences asked for fails, the context falls back to ONE sequence before it gives up.
    for (;;) {
        hipError_t e = hipSuccess;
        if (c->lbuf_cap < lbuf_bytes * (size_t)nseq) {
            if (c->d_lbuf) (void)hipFree(c->d_lbuf);
            c->d_lbuf = nullptr; c->lbuf_cap = 0;
            e = hipMalloc((void **)&c->d_lbuf, lbuf_bytes * (size_t)nseq);
            if (e == hipSuccess) {
                c->lbuf_cap = lbuf_bytes * (size_t)nseq;
                HIP_TRY(hipMemsetAsync(c->d_lbuf, 0, c->lbuf_cap, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                // (fresh planes: the serial numbers may start over as well)
                for (uint32_t sq = 0; sq < (uint32_t)PT_MAX_SEQUENCES; ++sq)
                    HIP_TRY(hipMemcpy(&c->d_state[sq].serial, &sq, sizeof sq, hipMemcpyHostToDevice));
                c->batches_stamped = 0;
            } else c->d_lbuf = nullptr;
        }
        if (e == hipSuccess && c->pool_cap < 2 * one * (size_t)nseq) {
            if (c->d_pool) (void)hipFree(c->d_pool);
            c->d_pool = nullptr; c->pool_cap = 0;
            e = hipMalloc(&c->d_pool, 2 * one * (size_t)nseq);
            if (e == hipSuccess) c->pool_cap = 2 * one * (size_t)nseq;
            else c->d_pool = nullptr;
        }
        if (e == hipSuccess) break;
        (void)hipGetLastError();
        if (nseq > 1) { nseq = 1; c->nseq = 1; continue; }      // (half the pools and planes)
        c->dirty = true;
        return fail(PT_ERR_OOM, "device memory: %zu B of ray pools + %zu B of radiance planes per launch sequence (%s)", 2 * one, lbuf_bytes,
                    hipGetErrorString(e));
    }
    k.lbuf = c->d_lbuf;
    for (int sq = 0; sq < PT_MAX_SEQUENCES; ++sq) {
        pt::KParams &ks = c->kps[sq];
        ks = k;
        if (sq >= nseq) continue;
        for (int q = 0; q < 2; ++q) {
            unsigned char *base = (unsigned char *)c->d_pool + (size_t)(2 * sq + q) * one;
            ks.pool[q].a = (float4 *)base;
            ks.pool[q].b = (float4 *)(base + slots * 16);
            ks.pool[q].c = (float2 *)(base + slots * 32);
        }
        ks.lbuf = (float *)((unsigned char *)c->d_lbuf + (size_t)sq * lbuf_bytes);
        ks.st = c->d_state + sq;
    }
    k = c->kps[0];
    if (getenv("PT_DEBUG_CLOCK")) fprintf(stderr, "[ptamd] launch sequences in flight: %d\n", nseq);
    return PT_OK;
}

// (re)build everything that depends on scene, camera or options: validate, build the scene tables on the host, upload them, choose
// the launch shape, then the span tables it takes and the memory of its launch sequences
int configure(pt_ctx *c)
{
    if (!c->have_scene) return fail(PT_ERR_INVALID, "pt_set_scene has not been called");
    if (!c->have_camera) return fail(PT_ERR_INVALID, "pt_set_camera has not been called");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dirty) return PT_OK;
    HIP_TRY(sync_all_streams(c));
    drop_graph(c);

    const pt_options &o = c->opt;
    const int W = (int)c->cam.resolution.x, H = (int)c->cam.resolution.y;
    if (W < 1 || H < 1) return fail(PT_ERR_INVALID, "camera resolution %dx%d", W, H);
    int r0 = o.row_begin, r1 = o.row_end;
    if (r0 == 0 && r1 == 0) r1 = H;
    if (r0 < 0 || r1 > H || r0 >= r1) return fail(PT_ERR_INVALID, "tile rows [%d,%d) outside frame height %d", r0, r1, H);
    int tile_rows = r1 - r0;
    if (o.strip_rows > 0) {
        tile_rows = pt_strip_local_rows(H, o.strip_rows, o.strip_world, o.strip_rank);
        if (tile_rows < 1) return fail(PT_ERR_INVALID, "rank %d of %d owns no strip of %d rows in a frame of height %d",
                                       o.strip_rank, o.strip_world, o.strip_rows, H);
    }
    const long long npix_ll = (long long)W * (long long)tile_rows;
    if ((long long)W * (long long)H > 0x7FFFFFFFLL / 4) return fail(PT_ERR_INVALID, "frame %dx%d too large", W, H);
    const int npix = (int)npix_ll;
    const size_t nGeoms = c->geoms.size(), nT = c->tri_geom.size();
    // motion blur with a shutter time per ray: knot states at shutter times j / slices (pt_tables.hip)
    const int nknots = motion_per_ray(c) ? c->motion_slices + 1 : 0;
    if (nknots > 0) {
        if (nT > 0) return fail(PT_ERR_INVALID, "motion_per_ray: triangle meshes need the slice scheme (motion_per_ray = 0)");
        for (const pt_static_geom &g : c->geoms)
            if (g.type == PT_MESH) return fail(PT_ERR_INVALID, "motion_per_ray: MESH objects need the slice scheme (motion_per_ray = 0)");
        if (o.compaction != 1) return fail(PT_ERR_INVALID, "motion_per_ray needs compaction 1 (got %d)", o.compaction);
        if (!(o.geom_path == 0 || o.geom_path == 1 || o.geom_path == 5))
            return fail(PT_ERR_INVALID, "motion_per_ray runs on the scalar and the pair-queue geometry paths (geom_path 0, 1 or 5, got %d)", o.geom_path);
        if (!(o.workgroup == 0 || o.workgroup == 256)) return fail(PT_ERR_INVALID, "motion_per_ray needs workgroup 0 or 256 (got %d)", o.workgroup);
    }

    const pt::SceneTables t = pt::build_tables({c->geoms, c->geoms_next, c->mats, c->tri_obj, c->tri_geom, c->cam,
                                                c->have_cam_next ? &c->cam_next : nullptr, o.lens_radius, nknots, c->motion_rotat});
    pt::KParams &k = c->kp;
    memset(&k, 0, sizeof k);
    pt::set_view(k, c->cam, o, W, r0, npix);
    k.nG = (int)(nGeoms + nT);
    k.ntri = (int)nT;
    k.ngeoms = (int)nGeoms;
    k.nM = (int)c->mats.size();
    k.depth = o.depth;
    k.rr_start = o.rr_start;
    k.seed = o.seed;
    k.nlights = o.direct_light ? (int)t.lights.size() : 0;
    k.absorption = o.absorption ? 1 : 0;
    k.scatter = o.scatter ? 1 : 0;
    k.slab_mask = nknots > 0 ? 0u : t.slab_mask;         // (a moving cube's slab moves with it)
    k.nknots = nknots;
    if (nknots > 0) { k.tan_x = pt::fov_tan(c->cam.fov.x); k.tan_y = pt::fov_tan(c->cam.fov.y); }
    k.nnodes = t.nnodes;
    k.nnodes4 = t.nnodes4;
    k.wdepth = t.wdepth;
    k.nbig = t.nbig;
    memcpy(k.big, t.big, sizeof k.big);
    k.eye_cull = getenv("PT_NO_EYE_CULL") ? 0 : 1;
    PT_TRY(upload_tables(c, t, k));

    // framebuffer
    const size_t img_bytes = (size_t)npix * 3 * sizeof(float);
    if (img_bytes != c->image_bytes) c->image_valid = false;
    c->image_bytes = img_bytes;
    if (!c->d_image_bound && c->image_cap < img_bytes) {
        if (c->d_image_own) (void)hipFree(c->d_image_own);
        c->d_image_own = nullptr; c->image_cap = 0;
        HIP_TRY(hipMalloc((void **)&c->d_image_own, img_bytes));
        c->image_cap = img_bytes;
        HIP_TRY(hipMemset(c->d_image_own, 0, img_bytes));
        c->image_valid = false;
    }
    k.image = image_ptr(c);
    k.st = c->d_state;

    PT_TRY(choose_launch(c, k));
    PT_TRY(upload_spans(c, t, k));
    PT_TRY(allocate_sequences(c, k));
    c->dirty = false;
    return PT_OK;
}

// one launch sequence = one batch of consecutive iterations (their number is device state, IterState::nslot):
// bookkeeping, depth bounce launches, accumulate.
// ev (optional): 2*depth events recorded around the bounce launches (pt_render_profiled).
// sq: the launch sequence (its pools, planes and IterState); with_accumulate = false leaves the accumulate to the caller,
// who orders it behind the previous batch's.
int bounce_launches_per_batch(const pt_ctx *c) { return c->cfg.resident ? 2 : c->kp.depth; }

// Serial numbers stamp the radiance-plane entries (32 bits, + PT_MAX_SEQUENCES per batch): long before they could come round
// again -- 2^29 batches of one context, weeks of rendering -- the planes are zeroed and the count starts over.  Every path that
// renders batches (pt_render, the ordered batches of the motion-blur slices, pt_render_profiled) books them here first.
// PT_SERIAL_BUDGET (environment, read once): a smaller budget, so that tests reach the restart (include/pt_abi.h, test hooks).
int book_batch_serials(pt_ctx *c, unsigned long long nb)
{
    static const unsigned long long serial_budget =
        (getenv("PT_SERIAL_BUDGET") && atoll(getenv("PT_SERIAL_BUDGET")) > 0) ? (unsigned long long)atoll(getenv("PT_SERIAL_BUDGET")) : (1ull << 29);
    if (c->batches_stamped + nb > serial_budget) {
        HIP_TRY(sync_all_streams(c));
        HIP_TRY(hipMemset(c->d_lbuf, 0, c->lbuf_cap));
        for (uint32_t sq = 0; sq < (uint32_t)PT_MAX_SEQUENCES; ++sq)
            HIP_TRY(hipMemcpy(&c->d_state[sq].serial, &sq, sizeof sq, hipMemcpyHostToDevice));
        c->batches_stamped = 0;
    }
    c->batches_stamped += nb;
    return PT_OK;
}

int enqueue_batch(pt_ctx *c, hipStream_t s, hipEvent_t *ev, int sq = 0, bool with_accumulate = true)
{
    const pt::KParams &kp = c->kps[sq];
    HIP_TRY(pt::launch_iter_begin(s, kp.st, kp.npix, kp.depth, c->cfg.compact));
    const int launches = bounce_launches_per_batch(c);      // (resident paths: the camera launch + one for all later bounces)
    for (int b = 0; b < launches; ++b) {
        if (ev) HIP_TRY(hipEventRecord(ev[2 * b], s));
        HIP_TRY(pt::launch_bounce(s, kp, c->cfg, b));
        if (ev) HIP_TRY(hipEventRecord(ev[2 * b + 1], s));
    }
    if (with_accumulate) HIP_TRY(pt::launch_accumulate(s, kp.image, kp.lbuf, kp.st, kp.npix));
    return PT_OK;
}

// iter_count iterations as near-equal batches of at most `batch`: n batches of q, the first r of them one more
// (20 iterations at batch 16 -> 10 + 10, not 16 + 4: a launch that carries 4 iterations pays the same fixed cost)
void batch_schedule(int iter_count, int batch, int *n, int *q, int *r)
{
    *n = (iter_count + batch - 1) / batch;
    *q = iter_count / *n;
    *r = iter_count % *n;
}

void drop_slices(pt_ctx *c)
{
    for (pt_ctx *k : c->slice_ctx) pt_destroy(k);
    c->slice_ctx.clear();
}

// motion blur: scene state of slice k of n = both frames interpolated at shutter time (k + .5)/n, component-wise in fp32
// as a + (b - a) * t on translation / rotation / scale (and the camera vectors), matrices rebuilt by the loader's
// buildTransformationMatrix (ref: src/utilities.cpp:74-90)
int build_slices(pt_ctx *c)
{
    if (!c->motion_dirty) return PT_OK;
    drop_slices(c);
    const int n = c->motion_slices;
    for (int k = 0; k < n; ++k) {
        pt_ctx *ch = nullptr;
        int rc = pt_create(c->device, &ch);
        if (rc != PT_OK) return rc;
        c->slice_ctx.push_back(ch);
        const float t = ((float)k + 0.5f) / (float)n;
        std::vector<pt_static_geom> g = c->geoms;
        for (size_t i = 0; i < g.size(); ++i) {
            const pt_static_geom &a = c->geoms[i], &b = c->geoms_next[i];
            g[i].translation = lerp3(a.translation, b.translation, t);
            g[i].rotation = lerp3(a.rotation, b.rotation, t);
            g[i].scale = lerp3(a.scale, b.scale, t);
            g[i].transform = ptamd::buildTransformationMatrix(g[i].translation, g[i].rotation, g[i].scale, c->motion_rotat, &g[i].inverseTransform);
        }
        pt_camera_data cam = c->cam;
        if (c->have_cam_next) {
            cam.position = lerp3(c->cam.position, c->cam_next.position, t);
            cam.view = lerp3(c->cam.view, c->cam_next.view, t);
            cam.up = lerp3(c->cam.up, c->cam_next.up, t);
        }
        rc = pt_set_options(ch, &c->opt);
        if (rc == PT_OK) rc = pt_set_scene(ch, g.data(), (int)g.size(), c->mats.data(), (int)c->mats.size());
        if (rc == PT_OK && !c->tri_geom.empty()) {
            // the same object-space triangles under the slice's transforms: one pt_mesh per run of triangles of one geom
            std::vector<pt_mesh> ms;
            for (size_t a0 = 0; a0 < c->tri_geom.size();) {
                size_t a1 = a0;
                while (a1 < c->tri_geom.size() && c->tri_geom[a1] == c->tri_geom[a0]) ++a1;
                ms.push_back(pt_mesh{c->tri_geom[a0], (int)(a1 - a0), c->tri_obj.data() + 9 * a0});
                a0 = a1;
            }
            rc = pt_set_meshes(ch, ms.data(), (int)ms.size());
        }
        if (rc == PT_OK) rc = pt_set_camera(ch, &cam);
        if (rc != PT_OK) return rc;
    }
    c->motion_dirty = false;
    return PT_OK;
}

// One batch (count <= the context's batch size) of context c on stream ss, for a caller that keeps several contexts busy on two
// streams (motion blur by slices): bookkeeping and bounce launches as soon as the stream gets to them, the accumulate behind
// `wait_ev` (the previous batch's accumulate, possibly on the other stream; nullptr: none), `done_ev` recorded behind it.
int render_batch_ordered(pt_ctx *c, hipStream_t ss, int iter_first, int count, hipEvent_t wait_ev, hipEvent_t done_ev)
{
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    if (count < 1 || count > c->batch) return fail(PT_ERR_INVALID, "render_batch_ordered: %d iterations (batch %d)", count, c->batch);
    rc = book_batch_serials(c, 1ull);
    if (rc != PT_OK) return rc;
    if (c->opt.use_graph && !c->graph_exec[0]) {        // slot 0: sequence 0's batch without its accumulate (as in pt_render)
        HIP_TRY(hipStreamBeginCapture(ss, hipStreamCaptureModeThreadLocal));
        rc = enqueue_batch(c, ss, nullptr, 0, false);
        hipError_t ce = hipStreamEndCapture(ss, &c->graph[0]);
        if (rc != PT_OK) { drop_graph(c); return rc; }
        if (ce != hipSuccess) { drop_graph(c); return fail(PT_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce)); }
        HIP_TRY(hipGraphInstantiate(&c->graph_exec[0], c->graph[0], nullptr, nullptr, 0));
    }
    HIP_TRY(pt::launch_iter_set(ss, c->d_state, (uint32_t)iter_first, (uint32_t)count, 0u, 0u, 1u));
    if (c->opt.use_graph) HIP_TRY(hipGraphLaunch(c->graph_exec[0], ss));
    else { rc = enqueue_batch(c, ss, nullptr, 0, false); if (rc != PT_OK) return rc; }
    if (wait_ev) HIP_TRY(hipStreamWaitEvent(ss, wait_ev, 0));
    const pt::KParams &ks = c->kps[0];
    HIP_TRY(pt::launch_accumulate(ss, ks.image, ks.lbuf, ks.st, ks.npix));
    HIP_TRY(pt::launch_iter_fold(ss, c->d_state, c->kp.depth));
    if (done_ev) HIP_TRY(hipEventRecord(done_ev, ss));
    c->bounce_launches += (unsigned long long)bounce_launches_per_batch(c);
    c->image_valid = true;
    return PT_OK;
}

}  // namespace

extern "C" {

const char *pt_last_error(void) { return g_last_error.c_str(); }
const char *pt_version(void) { return "ptamd 0.1 (gfx950, abi 2)"; }
int pt_abi_version(void) { return PT_ABI_VERSION; }
size_t pt_options_size(void) { return sizeof(pt_options); }

int pt_strip_local_rows(int height, int strip_rows, int world, int rank)
{
    if (height < 1 || strip_rows < 1 || world < 1 || rank < 0 || rank >= world) return 0;
    const long long nstrips = ((long long)height + strip_rows - 1) / strip_rows;      // the last one may be short
    long long rows = 0;
    for (long long k = rank; k < nstrips; k += world) {
        const long long left = (long long)height - k * strip_rows;
        rows += left < strip_rows ? left : strip_rows;
    }
    return (int)rows;
}

int pt_strip_global_row(int strip_rows, int world, int rank, int local_row)
{
    if (strip_rows < 1 || world < 1 || rank < 0 || rank >= world || local_row < 0) return -1;
    const int j = local_row / strip_rows, w = local_row % strip_rows;
    return (j * world + rank) * strip_rows + w;
}

int pt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void pt_default_options(pt_options *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->depth = 8;
    o->rr_start = -1;
    o->seed = 0;
    o->compaction = 1;
    o->workgroup = 0;
    o->geom_path = 0;
    o->use_graph = 1;
    o->batch = 0;
    o->lens_radius = 0.0f;
    o->focal_distance = 1.0f;
}

int pt_create(int device, pt_ctx **out)
{
    if (!out) return fail(PT_ERR_INVALID, "pt_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1)
        return fail(PT_ERR_NO_DEVICE, "no HIP device (%s); this renderer has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(PT_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PT_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 (MI355X) only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    pt_ctx *c = new pt_ctx();
    c->device = device;
    c->cu_count = prop.multiProcessorCount;
    pt_default_options(&c->opt);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(PT_ERR_HIP, "hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    if (hipMalloc((void **)&c->d_state, PT_MAX_SEQUENCES * sizeof(pt::IterState)) != hipSuccess ||
        hipMemset(c->d_state, 0, PT_MAX_SEQUENCES * sizeof(pt::IterState)) != hipSuccess) {
        pt_destroy(c);
        return fail(PT_ERR_OOM, "cannot allocate iteration state");
    }
    // batch serial numbers (the stamps of the radiance-plane entries): sequence q counts q + 4, q + 8, ... -- never zero, never
    // another sequence's, never one of its own again, so no entry an earlier batch left anywhere in the planes is ever mistaken
    for (uint32_t q = 1; q < (uint32_t)PT_MAX_SEQUENCES; ++q)
        if (hipMemcpy(&c->d_state[q].serial, &q, sizeof q, hipMemcpyHostToDevice) != hipSuccess) {
            pt_destroy(c);
            return fail(PT_ERR_HIP, "cannot initialise the iteration state");
        }
    *out = c;
    return PT_OK;
}

void pt_destroy(pt_ctx *c)
{
    if (!c) return;
    drop_slices(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)sync_all_streams(c);
    drop_graph(c);
    for (auto &t : c->timers) { (void)hipEventDestroy(t.first); (void)hipEventDestroy(t.second); }
    if (c->d_prims) (void)hipFree(c->d_prims);
    if (c->d_mats) (void)hipFree(c->d_mats);
    if (c->d_ro_eye) (void)hipFree(c->d_ro_eye);
    if (c->d_face_n) (void)hipFree(c->d_face_n);
    if (c->d_box_eye) (void)hipFree(c->d_box_eye);
    if (c->d_span_mask) (void)hipFree(c->d_span_mask);
    if (c->d_box_world) (void)hipFree(c->d_box_world);
    if (c->d_slab_n) (void)hipFree(c->d_slab_n);
    if (c->d_lights) (void)hipFree(c->d_lights);
    if (c->d_light_tris) (void)hipFree(c->d_light_tris);
    if (c->d_light_cdf) (void)hipFree(c->d_light_cdf);
    if (c->d_knots) (void)hipFree(c->d_knots);
    if (c->d_knot_cam) (void)hipFree(c->d_knot_cam);
    if (c->d_bvh) (void)hipFree(c->d_bvh);
    if (c->d_bvh4) (void)hipFree(c->d_bvh4);
    if (c->d_image_own) (void)hipFree(c->d_image_own);
    if (c->d_pool) (void)hipFree(c->d_pool);
    if (c->d_lbuf) (void)hipFree(c->d_lbuf);
    if (c->d_state) (void)hipFree(c->d_state);
    if (c->d_span_off) (void)hipFree(c->d_span_off);
    if (c->d_span_list) (void)hipFree(c->d_span_list);
    for (int q = 1; q < PT_MAX_SEQUENCES; ++q)
        if (c->seq_stream[q]) { (void)hipStreamSynchronize(c->seq_stream[q]); (void)hipStreamDestroy(c->seq_stream[q]); }
    for (int q = 0; q < PT_MAX_SEQUENCES; ++q)
        if (c->seq_acc[q]) (void)hipEventDestroy(c->seq_acc[q]);
    if (c->seq_fork) (void)hipEventDestroy(c->seq_fork);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int pt_set_options(pt_ctx *c, const pt_options *o)
{
    if (!c || !o) return fail(PT_ERR_INVALID, "pt_set_options: NULL argument");
    if (o->depth < 1 || o->depth > PT_MAX_DEPTH) return fail(PT_ERR_INVALID, "depth %d not in 1..%d", o->depth, PT_MAX_DEPTH);
    const int wg = o->workgroup;
    if (!(wg == 0 || wg == 64 || wg == 128 || wg == 256 || wg == 512 || wg == 1024))
        return fail(PT_ERR_INVALID, "workgroup %d not one of 0,64,128,256,512,1024", wg);
    if (o->geom_path < 0 || o->geom_path > 8) return fail(PT_ERR_INVALID, "geom_path %d not in 0..8", o->geom_path);
    if (o->row_begin < 0 || o->row_end < o->row_begin) return fail(PT_ERR_INVALID, "tile rows [%d,%d)", o->row_begin, o->row_end);
    if (o->strip_rows < 0 || (o->strip_rows > 0 && (o->strip_world < 1 || o->strip_rank < 0 || o->strip_rank >= o->strip_world)))
        return fail(PT_ERR_INVALID, "strips: rows %d, rank %d of %d", o->strip_rows, o->strip_rank, o->strip_world);
    if (o->strip_rows > 0 && (o->row_begin != 0 || o->row_end != 0))
        return fail(PT_ERR_INVALID, "strip tiles and a row band [%d,%d) exclude each other", o->row_begin, o->row_end);
    if (o->batch < 0 || o->batch > pt::PT_MAX_BATCH) return fail(PT_ERR_INVALID, "batch %d not in 0..%d", o->batch, pt::PT_MAX_BATCH);
    if (o->compaction < 0 || o->compaction > 2) return fail(PT_ERR_INVALID, "compaction %d not 0, 1 or 2", o->compaction);
    if (o->direct_light < 0 || o->direct_light > 1) return fail(PT_ERR_INVALID, "direct_light %d not 0 or 1", o->direct_light);
    if (o->absorption < 0 || o->absorption > 1) return fail(PT_ERR_INVALID, "absorption %d not 0 or 1", o->absorption);
    if (o->scatter < 0 || o->scatter > 1) return fail(PT_ERR_INVALID, "scatter %d not 0 or 1", o->scatter);
    if (!(o->lens_radius >= 0.0f) || (o->lens_radius > 0.0f && !(o->focal_distance > 0.0f)))
        return fail(PT_ERR_INVALID, "lens radius %g / focal distance %g", (double)o->lens_radius, (double)o->focal_distance);
    if (o->motion_per_ray < 0 || o->motion_per_ray > 1) return fail(PT_ERR_INVALID, "motion_per_ray %d not 0 or 1", o->motion_per_ray);
    if (o->sequences < 0 || o->sequences > PT_MAX_SEQUENCES) return fail(PT_ERR_INVALID, "sequences %d not in 0..%d", o->sequences, PT_MAX_SEQUENCES);
    if (o->resident < -1 || o->resident > 1) return fail(PT_ERR_INVALID, "resident %d not -1, 0 or 1", o->resident);
    if (o->direct_light && o->compaction != 1) return fail(PT_ERR_INVALID, "direct_light needs compaction 1 (got %d)", o->compaction);
    if (o->scatter && o->compaction != 1) return fail(PT_ERR_INVALID, "scatter needs compaction 1 (got %d)", o->compaction);
    c->opt = *o;
    c->dirty = true;
    c->motion_dirty = c->motion_slices >= 1;
    return PT_OK;
}

int pt_get_options(pt_ctx *c, pt_options *o)
{
    if (!c || !o) return fail(PT_ERR_INVALID, "pt_get_options: NULL argument");
    *o = c->opt;
    return PT_OK;
}

int pt_set_scene(pt_ctx *c, const pt_static_geom *geoms, int nG, const pt_material *mats, int nM)
{
    if (!c || nG < 0 || nM < 0 || (nG > 0 && !geoms) || (nM > 0 && !mats))
        return fail(PT_ERR_INVALID, "pt_set_scene: bad arguments (nG=%d nM=%d)", nG, nM);
    for (int i = 0; i < nG; ++i) {
        if (geoms[i].type < PT_SPHERE || geoms[i].type > PT_MESH)
            return fail(PT_ERR_INVALID, "geom %d: type %d is not SPHERE/CUBE/MESH", i, geoms[i].type);
        if (geoms[i].type != PT_MESH && (geoms[i].materialid < 0 || geoms[i].materialid >= nM))
            return fail(PT_ERR_INVALID, "geom %d: materialid %d outside 0..%d", i, geoms[i].materialid, nM - 1);
    }
    c->geoms.assign(geoms, geoms + nG);
    c->mats.assign(mats, mats + nM);
    c->tri_obj.clear();
    c->tri_geom.clear();
    c->geoms_next.clear();                 // motion blur belongs to the scene it was set for
    c->motion_slices = 0;
    drop_slices(c);
    c->have_scene = true;
    c->dirty = true;
    return PT_OK;
}

int pt_set_meshes(pt_ctx *c, const pt_mesh *meshes, int n)
{
    if (!c || n < 0 || (n > 0 && !meshes)) return fail(PT_ERR_INVALID, "pt_set_meshes: bad arguments (n=%d)", n);
    if (!c->have_scene) return fail(PT_ERR_INVALID, "pt_set_meshes: call pt_set_scene first");
    std::vector<float> tri;
    std::vector<int> owner;
    for (int k = 0; k < n; ++k) {
        const pt_mesh &m = meshes[k];
        if (m.geom < 0 || m.geom >= (int)c->geoms.size() || c->geoms[(size_t)m.geom].type != PT_MESH)
            return fail(PT_ERR_INVALID, "mesh %d: geom %d is not a MESH object", k, m.geom);
        if (m.n_triangles < 0 || (m.n_triangles > 0 && !m.vertices)) return fail(PT_ERR_INVALID, "mesh %d: %d triangles, no vertices", k, m.n_triangles);
        const int mat = c->geoms[(size_t)m.geom].materialid;
        if (m.n_triangles > 0 && (mat < 0 || mat >= (int)c->mats.size()))
            return fail(PT_ERR_INVALID, "mesh %d: materialid %d of geom %d outside 0..%d", k, mat, m.geom, (int)c->mats.size() - 1);
        tri.insert(tri.end(), m.vertices, m.vertices + 9 * (size_t)m.n_triangles);
        owner.insert(owner.end(), (size_t)m.n_triangles, m.geom);
    }
    c->tri_obj.swap(tri);
    c->tri_geom.swap(owner);
    c->dirty = true;
    c->motion_dirty = c->motion_slices >= 1;
    return PT_OK;
}

int pt_set_motion(pt_ctx *c, const pt_static_geom *geoms_next, const pt_camera_data *cam_next, int slices, int rotat_units)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_set_motion: NULL context");
    if (slices < 1 || !geoms_next) {                     // motion off
        c->motion_slices = 0;
        c->geoms_next.clear();
        c->have_cam_next = false;
        drop_slices(c);
        c->dirty = true;
        return PT_OK;
    }
    if (!c->have_scene || !c->have_camera) return fail(PT_ERR_INVALID, "pt_set_motion: call pt_set_scene and pt_set_camera first");
    if (slices > 64) return fail(PT_ERR_INVALID, "pt_set_motion: %d slices (at most 64)", slices);
    if (rotat_units != PT_ROTAT_RADIANS && rotat_units != PT_ROTAT_DEGREES) return fail(PT_ERR_INVALID, "pt_set_motion: rotat_units %d", rotat_units);
    for (size_t i = 0; i < c->geoms.size(); ++i)
        if (geoms_next[i].type != c->geoms[i].type || geoms_next[i].materialid != c->geoms[i].materialid)
            return fail(PT_ERR_INVALID, "pt_set_motion: object %d changes type or material between the frames", (int)i);
    c->geoms_next.assign(geoms_next, geoms_next + c->geoms.size());
    c->have_cam_next = cam_next != nullptr;
    if (cam_next) c->cam_next = *cam_next;
    c->motion_slices = slices;
    c->motion_rotat = rotat_units;
    c->motion_dirty = true;
    c->dirty = true;                                      // (per-ray mode: the knots are part of the configuration)
    return PT_OK;
}

int pt_set_camera(pt_ctx *c, const pt_camera_data *cam)
{
    if (!c || !cam) return fail(PT_ERR_INVALID, "pt_set_camera: NULL argument");
    if (!(cam->resolution.x >= 1.0f) || !(cam->resolution.y >= 1.0f))
        return fail(PT_ERR_INVALID, "camera resolution %gx%g", cam->resolution.x, cam->resolution.y);
    c->cam = *cam;
    c->have_camera = true;
    c->dirty = true;
    c->motion_dirty = c->motion_slices >= 1;
    return PT_OK;
}

int pt_set_stream(pt_ctx *c, void *hip_stream)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_set_stream: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_all_streams(c));
    if (fold_timers(c) != PT_OK) return PT_ERR_HIP;
    drop_graph(c);
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PT_OK;
}

size_t pt_image_bytes(pt_ctx *c)
{
    if (!c || !c->have_camera) return 0;
    const int W = (int)c->cam.resolution.x, H = (int)c->cam.resolution.y;
    int r0 = c->opt.row_begin, r1 = c->opt.row_end;
    if (r0 == 0 && r1 == 0) r1 = H;
    if (r1 > H || r0 >= r1) return 0;
    int rows = r1 - r0;
    if (c->opt.strip_rows > 0) rows = pt_strip_local_rows(H, c->opt.strip_rows, c->opt.strip_world, c->opt.strip_rank);
    if (rows < 1) return 0;
    return (size_t)W * (size_t)rows * 3 * sizeof(float);
}

int pt_bind_image(pt_ctx *c, void *device_rgb)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_bind_image: NULL context");
    c->d_image_bound = (float *)device_rgb;
    c->image_valid = false;
    c->dirty = true;
    return PT_OK;
}

int pt_image_device_pointer(pt_ctx *c, void **out)
{
    if (!c || !out) return fail(PT_ERR_INVALID, "pt_image_device_pointer: NULL argument");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    *out = image_ptr(c);
    return PT_OK;
}

int pt_clear_image(pt_ctx *c)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_clear_image: NULL context");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    HIP_TRY(hipMemsetAsync(image_ptr(c), 0, c->image_bytes, c->stream));
    c->image_valid = false;
    return PT_OK;
}

int pt_upload_image(pt_ctx *c, const float *host_rgb)
{
    if (!c || !host_rgb) return fail(PT_ERR_INVALID, "pt_upload_image: NULL argument");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(image_ptr(c), host_rgb, c->image_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->image_valid = true;
    return PT_OK;
}

int pt_download_image(pt_ctx *c, float *host_rgb)
{
    if (!c || !host_rgb) return fail(PT_ERR_INVALID, "pt_download_image: NULL argument");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(host_rgb, image_ptr(c), c->image_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_render(pt_ctx *c, int iter_first, int iter_count)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_render: NULL context");
    if (iter_first < 1 || iter_count < 0) return fail(PT_ERR_INVALID, "pt_render: iterations [%d,+%d)", iter_first, iter_count);
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    if (iter_count == 0) return PT_OK;
    hipStream_t s = c->stream;
    if (!motion_by_slices(c) && !c->slice_ctx.empty()) drop_slices(c);      // (left over from the slice scheme)
    if (motion_by_slices(c)) {
        // motion blur: every run of PT_SLICE_ITERATIONS iterations belongs to one shutter slice, rendered by that
        // slice's context into this context's framebuffer (the running mean is stateless given image and iteration)
        rc = build_slices(c);
        if (rc != PT_OK) return rc;
        for (pt_ctx *ch : c->slice_ctx) {
            if (ch->d_image_bound != image_ptr(c)) { rc = pt_bind_image(ch, image_ptr(c)); if (rc != PT_OK) return rc; }
            if (ch->stream != s) { rc = pt_set_stream(ch, (void *)s); if (rc != PT_OK) return rc; }
        }
        // Consecutive runs belong to different slices -- different contexts with pools of their own --, so they alternate
        // between the render stream and a second one like the launch sequences of a static scene do: a run's launches fill
        // the tails of its neighbour's, only the accumulates into the shared framebuffer are chained (iteration order).
        // (A child whose batch is smaller than a run -- huge tiles -- takes the plain, serial path.)
        bool two_streams = c->nseq > 1;
        for (pt_ctx *ch : c->slice_ctx) {
            rc = configure(ch);
            if (rc != PT_OK) return rc;
            if (ch->batch < PT_SLICE_ITERATIONS) two_streams = false;
        }
        if (two_streams) {
            if (!c->seq_stream[1]) HIP_TRY(hipStreamCreateWithFlags(&c->seq_stream[1], hipStreamNonBlocking));
            for (int sq = 0; sq < 2; ++sq)
                if (!c->seq_acc[sq]) HIP_TRY(hipEventCreateWithFlags(&c->seq_acc[sq], hipEventDisableTiming | hipEventDisableSystemFence));
            if (!c->seq_fork) HIP_TRY(hipEventCreateWithFlags(&c->seq_fork, hipEventDisableTiming | hipEventDisableSystemFence));
            if (c->timers.size() >= 1024) { rc = fold_timers(c); if (rc != PT_OK) return rc; }
            hipEvent_t e0, e1;
            HIP_TRY(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));
            HIP_TRY(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
            c->timers.emplace_back(e0, e1);
            HIP_TRY(hipEventRecord(e0, s));
            HIP_TRY(hipEventRecord(c->seq_fork, s));
            HIP_TRY(hipStreamWaitEvent(c->seq_stream[1], c->seq_fork, 0));
            int j = 0;
            for (int it = iter_first; it < iter_first + iter_count; ++j) {
                const int run = (it - 1) / PT_SLICE_ITERATIONS;
                int end = (run + 1) * PT_SLICE_ITERATIONS + 1;
                if (end > iter_first + iter_count) end = iter_first + iter_count;
                hipStream_t ss = (j & 1) ? c->seq_stream[1] : s;
                rc = render_batch_ordered(c->slice_ctx[(size_t)(run % c->motion_slices)], ss, it, end - it,
                                          j > 0 ? c->seq_acc[(j - 1) & 1] : nullptr, c->seq_acc[j & 1]);
                if (rc != PT_OK) { (void)sync_all_streams(c); c->image_valid = false; return rc; }      // (nothing keeps running on the second stream)
                it = end;
            }
            if (j > 1) HIP_TRY(hipStreamWaitEvent(s, c->seq_acc[1], 0));        // join (the last event of the second stream)
            HIP_TRY(hipEventRecord(e1, s));
            c->image_valid = true;
            return PT_OK;
        }
        for (int it = iter_first; it < iter_first + iter_count;) {
            const int run = (it - 1) / PT_SLICE_ITERATIONS;
            int end = (run + 1) * PT_SLICE_ITERATIONS + 1;
            if (end > iter_first + iter_count) end = iter_first + iter_count;
            rc = pt_render(c->slice_ctx[(size_t)(run % c->motion_slices)], it, end - it);
            if (rc != PT_OK) return rc;
            it = end;
        }
        c->image_valid = true;
        return PT_OK;
    }

    int nb, q, r;
    batch_schedule(iter_count, c->batch, &nb, &q, &r);
    // sequences actually used by this call (a call of one batch runs on sequence 0 alone)
    const int nseq = nb < c->nseq ? nb : c->nseq;
    const bool own_acc = nseq > 1;       // the accumulates are ordered across the sequences by events, outside the graphs
    c->seq_stream[0] = s;
    if (c->nseq > 1) {
        for (int sq = 1; sq < c->nseq; ++sq)
            if (!c->seq_stream[sq]) HIP_TRY(hipStreamCreateWithFlags(&c->seq_stream[sq], hipStreamNonBlocking));
        for (int sq = 0; sq < c->nseq; ++sq)
            if (!c->seq_acc[sq]) HIP_TRY(hipEventCreateWithFlags(&c->seq_acc[sq], hipEventDisableTiming | hipEventDisableSystemFence));
        if (!c->seq_fork) HIP_TRY(hipEventCreateWithFlags(&c->seq_fork, hipEventDisableTiming | hipEventDisableSystemFence));
    }
    if (c->opt.use_graph) {
        // every graph this configuration can replay is captured by its first pt_render, whatever that call's size: slots
        // [0, nseq) = a sequence's batch without the accumulate, slot PT_MAX_SEQUENCES = sequence 0's with it (one-batch
        // calls) -- a later, longer call then meets no capture / instantiate (milliseconds of host time) on its way
        for (int gs = 0; gs <= PT_MAX_SEQUENCES; ++gs) {
            const bool whole = gs == PT_MAX_SEQUENCES;
            if ((!whole && (c->nseq < 2 || gs >= c->nseq)) || c->graph_exec[gs]) continue;
            const int sq = whole ? 0 : gs;
            hipStream_t ss = c->seq_stream[sq];
            HIP_TRY(hipStreamBeginCapture(ss, hipStreamCaptureModeThreadLocal));
            rc = enqueue_batch(c, ss, nullptr, sq, whole);
            hipError_t ce = hipStreamEndCapture(ss, &c->graph[gs]);
            if (rc != PT_OK) { drop_graph(c); return rc; }
            if (ce != hipSuccess) { drop_graph(c); return fail(PT_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce)); }
            HIP_TRY(hipGraphInstantiate(&c->graph_exec[gs], c->graph[gs], nullptr, nullptr, 0));
        }
    }
    rc = book_batch_serials(c, (unsigned long long)nb);
    if (rc != PT_OK) return rc;
    if (c->timers.size() >= 1024) { rc = fold_timers(c); if (rc != PT_OK) return rc; }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));
    HIP_TRY(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
    c->timers.emplace_back(e0, e1);
    HIP_TRY(hipEventRecord(e0, s));

    // fork ... join: a failure in between must not leave a side stream running (it would still touch the pools, the planes and
    // the shared framebuffer while the caller reconfigures or frees them): the lambda's error returns land in the wait below
    auto forked = [&]() -> int {
        if (nseq > 1) {
            // fork: the other sequences start behind everything already on the render stream
            HIP_TRY(hipEventRecord(c->seq_fork, s));
            for (int sq = 1; sq < nseq; ++sq) HIP_TRY(hipStreamWaitEvent(c->seq_stream[sq], c->seq_fork, 0));
        }
        for (int sq = 0; sq < nseq; ++sq)
            HIP_TRY(pt::launch_iter_set(c->seq_stream[sq], c->d_state + sq, (uint32_t)iter_first, (uint32_t)q, (uint32_t)r, (uint32_t)sq, (uint32_t)nseq));
        for (int i = 0; i < nb; ++i) {
            const int sq = i % nseq;
            hipStream_t ss = c->seq_stream[sq];
            if (c->opt.use_graph) {
                const int gs = own_acc ? sq : PT_MAX_SEQUENCES;       // (a one-batch call runs on sequence 0 with its accumulate)
                HIP_TRY(hipGraphLaunch(c->graph_exec[gs], ss));
            } else {
                const int rc2 = enqueue_batch(c, ss, nullptr, sq, !own_acc);
                if (rc2 != PT_OK) return rc2;
            }
            if (own_acc) {
                // the running mean takes the batches in iteration order: batch i's accumulate behind batch i - 1's
                if (i > 0) HIP_TRY(hipStreamWaitEvent(ss, c->seq_acc[(i - 1) % nseq], 0));
                const pt::KParams &ks = c->kps[sq];
                HIP_TRY(pt::launch_accumulate(ss, ks.image, ks.lbuf, ks.st, ks.npix));
                HIP_TRY(hipEventRecord(c->seq_acc[sq], ss));
            }
        }
        for (int sq = 0; sq < nseq; ++sq) HIP_TRY(pt::launch_iter_fold(c->seq_stream[sq], c->d_state + sq, c->kp.depth));
        if (nseq > 1) {
            // join: the render stream continues behind every sequence
            for (int sq = 1; sq < nseq; ++sq) {
                HIP_TRY(hipEventRecord(c->seq_acc[sq], c->seq_stream[sq]));
                HIP_TRY(hipStreamWaitEvent(s, c->seq_acc[sq], 0));
            }
        }
        HIP_TRY(hipEventRecord(e1, s));
        return PT_OK;
    };
    rc = forked();
    if (rc != PT_OK) {
        (void)sync_all_streams(c);
        c->image_valid = false;
        return rc;
    }
    c->bounce_launches += (unsigned long long)nb * (unsigned long long)bounce_launches_per_batch(c);
    c->image_valid = true;
    return PT_OK;
}

int pt_get_launch_info(pt_ctx *c, pt_launch_info *out)
{
    if (!c || !out) return fail(PT_ERR_INVALID, "pt_get_launch_info: NULL argument");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    memset(out, 0, sizeof *out);
    out->geom_path = c->cfg.geom + 1;
    out->workgroup = c->cfg.workgroup;
    out->grid = c->cfg.grid;
    out->batch = c->batch;
    out->sequences = c->nseq;
    out->resident = c->cfg.resident;
    out->refill_min = c->kp.refill_min;
    out->launches_per_batch = bounce_launches_per_batch(c);
    out->lds_bytes = (int)pt::bounce_lds_bytes(c->kp, c->cfg);
    out->slab_pretest = c->cfg.slab;
    return PT_OK;
}

int pt_render_profiled(pt_ctx *c, int iter_first, int iter_count, double *bounce_ms_out)
{
    if (!c || !bounce_ms_out) return fail(PT_ERR_INVALID, "pt_render_profiled: NULL argument");
    if (iter_first < 1 || iter_count < 0) return fail(PT_ERR_INVALID, "pt_render_profiled: iterations [%d,+%d)", iter_first, iter_count);
    if (motion_by_slices(c)) return fail(PT_ERR_INVALID, "pt_render_profiled: not with motion blur by slices (profile a slice's scene instead)");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    const int depth = c->kp.depth;
    for (int b = 0; b < depth; ++b) bounce_ms_out[b] = 0.0;
    if (iter_count == 0) return PT_OK;
    hipStream_t s = c->stream;
    std::vector<hipEvent_t> ev((size_t)2 * (size_t)depth, nullptr);
    // (every exit below destroys the events that exist)
    struct EventGuard {
        std::vector<hipEvent_t> &ev;
        ~EventGuard() { for (auto &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
    } guard{ev};
    // no system-scope fence at the events: a default event makes every kernel end with an L2 write-back and start with
    // a cold cache, which showed up as +12 % on the launches bracketed this way
    for (auto &e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    int nb, q, r;
    batch_schedule(iter_count, c->batch, &nb, &q, &r);
    rc = book_batch_serials(c, (unsigned long long)nb);
    if (rc != PT_OK) return rc;
    HIP_TRY(pt::launch_iter_set(s, c->d_state, (uint32_t)iter_first, (uint32_t)q, (uint32_t)r, 0u, 1u));
    int launches = 0;
    for (int i = 0; i < nb; ++i) {
        rc = enqueue_batch(c, s, ev.data());
        if (rc != PT_OK) { (void)hipStreamSynchronize(s); return rc; }
        launches++;
        HIP_TRY(hipStreamSynchronize(s));
        for (int b = 0; b < bounce_launches_per_batch(c); ++b) {      // (resident paths: [1] = the one launch of all later bounces)
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 * b], ev[2 * b + 1]));
            bounce_ms_out[b] += (double)ms;
        }
    }
    HIP_TRY(pt::launch_iter_fold(s, c->d_state, depth));
    HIP_TRY(hipStreamSynchronize(s));
    c->bounce_launches += (unsigned long long)launches * (unsigned long long)bounce_launches_per_batch(c);
    c->image_valid = true;
    return PT_OK;
}

int pt_selftest_math(pt_ctx *c, unsigned long long mismatches_out[3])
{
    if (!c || !mismatches_out) return fail(PT_ERR_INVALID, "pt_selftest_math: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, 3 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = pt::launch_selftest_math(c->stream, d);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(mismatches_out, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(PT_ERR_HIP, "pt_selftest_math: %s", hipGetErrorString(e));
    return PT_OK;
}

int pt_device_kat(pt_ctx *c, int op, const float *in, int n_in, float *out, int n_out)
{
    if (!c || !in || !out || n_in < 1 || n_out < 1 || n_in > 4096 || n_out > 4096)
        return fail(PT_ERR_INVALID, "pt_device_kat: bad arguments");
    static const int need_in[] = {0, 1, 1, 5, 39, 5, 16, 17, 17, 20, 7, 6, 8, 11, 4, 18, 1, 17, 11};
    if (op < 1 || op > 18 || n_in < need_in[op]) return fail(PT_ERR_INVALID, "pt_device_kat: op %d needs %d inputs", op, op >= 1 && op <= 18 ? need_in[op] : 0);
    HIP_TRY(hipSetDevice(c->device));
    float *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, (size_t)(n_in + n_out) * sizeof(float)));
    hipError_t e = hipMemcpy(d, in, (size_t)n_in * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d + n_in, 0, (size_t)n_out * sizeof(float));
    if (e == hipSuccess) e = pt::launch_device_kat(c->stream, op, d, d + n_in, n_out);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d + n_in, (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(PT_ERR_HIP, "pt_device_kat: %s", hipGetErrorString(e));
    return PT_OK;
}

int pt_send_image_to_pbo(pt_ctx *c, pt_uchar4 *device_pbo)
{
    if (!c || !device_pbo) return fail(PT_ERR_INVALID, "pt_send_image_to_pbo: NULL argument");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    HIP_TRY(pt::launch_send_image_to_pbo(c->stream, device_pbo, image_ptr(c), c->kp.npix));
    return PT_OK;
}

int pt_record_event(pt_ctx *c, void *hip_event)
{
    if (!c || !hip_event) return fail(PT_ERR_INVALID, "pt_record_event: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord((hipEvent_t)hip_event, c->stream));
    return PT_OK;
}

int pt_synchronize(pt_ctx *c)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_synchronize: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_all_streams(c));
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_render_iteration(pt_ctx *c, pt_uchar4 *pbo, float *host_image, int iteration)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_render_iteration: NULL context");
    int rc = configure(c);
    if (rc != PT_OK) return rc;
    // The running mean is stateless given (image, iteration) (ref: src/raytraceKernel.cu:120,154): a context
    // that has not rendered iterations 1..iteration-1 itself takes them from the caller's buffer.
    if (iteration > 1 && !c->image_valid && host_image) {
        rc = pt_upload_image(c, host_image);
        if (rc != PT_OK) return rc;
    }
    rc = pt_render(c, iteration, 1);
    if (rc != PT_OK) return rc;
    if (pbo) { rc = pt_send_image_to_pbo(c, pbo); if (rc != PT_OK) return rc; }
    if (host_image) return pt_download_image(c, host_image);
    return pt_synchronize(c);
}

int pt_get_stats(pt_ctx *c, pt_stats *out)
{
    if (!c || !out) return fail(PT_ERR_INVALID, "pt_get_stats: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_all_streams(c));
    int rc = fold_timers(c);
    if (rc != PT_OK) return rc;
    pt::IterState h;
    HIP_TRY(hipMemcpy(&h, c->d_state, sizeof h, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->iterations = h.iterations;
    for (int b = 0; b < PT_MAX_DEPTH; ++b) { out->live_in[b] = h.live_in[b]; out->ray_bounces += h.live_in[b]; }
    for (int sq = 1; sq < PT_MAX_SEQUENCES; ++sq) {         // the other launch sequences' counts (diagnostics: sequence 0's)
        pt::IterState h2;
        HIP_TRY(hipMemcpy(&h2, c->d_state + sq, sizeof h2, hipMemcpyDeviceToHost));
        out->iterations += h2.iterations;
        for (int b = 0; b < PT_MAX_DEPTH; ++b) { out->live_in[b] += h2.live_in[b]; out->ray_bounces += h2.live_in[b]; }
        h.shadow_rays += h2.shadow_rays;
    }
    out->gpu_ms = c->gpu_ms;
    if (getenv("PT_DEBUG_CLOCK")) fprintf(stderr, "[ptamd] cull: tested %llu skipped %llu (wave x primitive)\n", h.clk[2], h.clk[3]);
    if (getenv("PT_DEBUG_CLOCK") && h.clk[1])
        fprintf(stderr, "[ptamd] bounce-1 workgroup 0: %llu shader clocks in %llu x 10 ns -> %.0f MHz\n", h.clk[0], h.clk[1],
                (double)h.clk[0] / (double)h.clk[1] * 100.0);
    if (getenv("PT_DEBUG_SPAN") && atoi(getenv("PT_DEBUG_SPAN")) == 2) {     // -DPT_DEBUG_SPAN=2 builds
        fprintf(stderr, "[ptamd] bounce-1 workgroup lifetime sums by blockIdx %% 8 (10 ns ticks):");
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %llu", h.dbg[x]);
        fprintf(stderr, "\n");
    } else if (getenv("PT_DEBUG_SPAN") && h.dbg[1])                          // -DPT_DEBUG_SPAN=1 builds
        fprintf(stderr, "[ptamd] bounce-1 workgroups: %llu lifetimes, mean %.1f us, shortest %.1f us, longest %.1f us; first start to last end over all launches %.1f us\n",
                h.dbg[1], (double)h.dbg[0] / (double)h.dbg[1] * 0.01, (double)(~h.dbg[3]) * 0.01, (double)h.dbg[2] * 0.01,
                (double)(h.dbg[5] - ~h.dbg[4]) * 0.01);
    out->bounce_launches = c->bounce_launches;
    out->shadow_rays = h.shadow_rays;
    for (pt_ctx *ch : c->slice_ctx) {                    // motion blur: the slices did the work
        pt_stats cs;
        rc = pt_get_stats(ch, &cs);
        if (rc != PT_OK) return rc;
        out->iterations += cs.iterations;
        out->ray_bounces += cs.ray_bounces;
        for (int b = 0; b < PT_MAX_DEPTH; ++b) out->live_in[b] += cs.live_in[b];
        out->gpu_ms += cs.gpu_ms;
        out->bounce_launches += cs.bounce_launches;
        out->shadow_rays += cs.shadow_rays;
    }
    if (getenv("PT_DEBUG_PHASE") && h.dbg[3] && h.dbg[7])
        fprintf(stderr, "[ptamd] shader clocks per chunk (wave latency): bounce 0: load/gen %.0f, nearest hit %.0f, shade+write %.0f; later: %.0f, %.0f, %.0f\n",
                (double)h.dbg[0] / h.dbg[3], (double)h.dbg[1] / h.dbg[3], (double)h.dbg[2] / h.dbg[3],
                (double)h.dbg[4] / h.dbg[7], (double)h.dbg[5] / h.dbg[7], (double)h.dbg[6] / h.dbg[7]);
    if (getenv("PT_DEBUG_BOUNDS") && h.dbg[0])
        fprintf(stderr, "[ptamd] BOUNDS violation: code %llu value %llu limit %llu block %llu thread %llu\n", h.dbg[0], h.dbg[1], h.dbg[2], h.dbg[4], h.dbg[5]);
    if (getenv("PT_DEBUG_PHASE2") && h.dbg[7])
        fprintf(stderr, "[ptamd] later bounces, shader clocks per chunk: load %.0f | nearest hit %.0f (pre-test + full batches %.0f, last batches %.0f, "
                        "result %.0f) | shade + radiance write %.0f | compaction + pool write %.0f\n",
                (double)h.dbg[0] / h.dbg[7], (double)h.dbg[3] / h.dbg[7], (double)h.dbg[1] / h.dbg[7], (double)h.dbg[2] / h.dbg[7],
                ((double)h.dbg[3] - (double)h.dbg[1] - (double)h.dbg[2]) / h.dbg[7], (double)h.dbg[4] / h.dbg[7], (double)h.dbg[5] / h.dbg[7]);
    if (getenv("PT_DEBUG_PHASE2") && h.lane_budget[13]) {
        // the lane budget of the later bounces (pair path): where the wave's clocks go and how many of the 64 lanes had work there
        const unsigned long long *B = h.lane_budget;
        const double rounds = (double)B[13];
        struct { const char *name; double clk, lane_clk; } ph[7] = {
            {"load / refill", (double)B[0], (double)B[1]}, {"pre-test loop", (double)B[2], (double)B[3]}, {"full batches", (double)B[4], (double)B[4] * 64.0},
            {"last batches", (double)B[5], (double)B[6]}, {"result", (double)B[7], (double)B[8]}, {"shade + radiance write", (double)B[9], (double)B[10]},
            {"compaction / hand-over", (double)B[11], (double)B[12]}};
        double tot = 0.0, tot_lane = 0.0;
        for (auto &x : ph) { tot += x.clk; tot_lane += x.lane_clk; }
        fprintf(stderr, "[ptamd] lane budget, later bounces: %.0f trips, %.1f rays per trip, %.0f clocks per trip; lanes with work, clock-weighted: %.1f of 64\n",
                rounds, (double)B[14] / rounds, tot / rounds, tot_lane / tot);
        fprintf(stderr, "[ptamd]   %-26s %10s %8s %12s %14s\n", "phase", "clocks/trip", "share", "busy lanes", "idle share");
        for (auto &x : ph)
            fprintf(stderr, "[ptamd]   %-26s %10.0f %7.1f%% %12.1f %13.1f%%\n", x.name, x.clk / rounds, 100.0 * x.clk / tot, x.clk > 0 ? x.lane_clk / x.clk : 0.0,
                    100.0 * (x.clk * 64.0 - x.lane_clk) / (tot * 64.0));
    }
    if (getenv("PT_DEBUG_PAIR") && h.dbg[4])
        fprintf(stderr, "[ptamd] pair queue: per ray %.2f sphere + %.2f box pairs; candidates that hit: %.2f + %.2f per ray; batches per wave round %.2f\n",
                (double)h.dbg[0] / h.dbg[4], (double)h.dbg[1] / h.dbg[4], (double)h.dbg[2] / h.dbg[4], (double)h.dbg[3] / h.dbg[4], (double)h.dbg[5] / h.dbg[6]);
    if (getenv("PT_DEBUG_CLOCK") && h.dbg[2])
        fprintf(stderr, "[ptamd] hierarchy walk: %.1f nodes, %.2f leaves per ray; per wave (longest lane): %.1f nodes, %.2f leaves, %.2f rounds\n",
                (double)h.dbg[0] / (double)h.dbg[2], (double)h.dbg[1] / (double)h.dbg[2], (double)h.dbg[3] / (double)h.dbg[6],
                (double)h.dbg[4] / (double)h.dbg[6], (double)h.dbg[5] / (double)h.dbg[6]);
    if (getenv("PT_DEBUG_W4") && h.dbg[2] && h.dbg[3] && h.dbg[6])
        fprintf(stderr, "[ptamd] batched walk: %.2f entries per ray, %.1f steps per wave round, %.1f entries per step, %.1f pairs per round\n",
                (double)h.dbg[0] / (double)h.dbg[2], (double)h.dbg[3] / (double)h.dbg[6], (double)h.dbg[0] / (double)h.dbg[3],
                (double)h.dbg[7] / (double)h.dbg[6]);
    if (getenv("PT_DEBUG_CLOCK") && h.dbg[7]) fprintf(stderr, "[ptamd] pairs per wave round: %.1f\n", (double)h.dbg[7] / (double)h.dbg[6]);
    return PT_OK;
}

int pt_reset_stats(pt_ctx *c)
{
    if (!c) return fail(PT_ERR_INVALID, "pt_reset_stats: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(sync_all_streams(c));
    int rc = fold_timers(c);
    if (rc != PT_OK) return rc;
    // (everything behind the header: the header holds the batch serial number, which outlives the statistics)
    for (int sq = 0; sq < PT_MAX_SEQUENCES; ++sq)
        HIP_TRY(hipMemset((unsigned char *)(c->d_state + sq) + offsetof(pt::IterState, counts), 0, sizeof(pt::IterState) - offsetof(pt::IterState, counts)));
    c->gpu_ms = 0.0;
    c->bounce_launches = 0;
    for (pt_ctx *ch : c->slice_ctx) { rc = pt_reset_stats(ch); if (rc != PT_OK) return rc; }
    return PT_OK;
}

}  // extern "C"
