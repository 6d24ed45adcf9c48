// context.h -- the handle behind the C ABI (tcsfm_ctx) and what every entry point and driver uses around it: DeviceGuard, HIPCHK, RESERVE,
// fail, the overlap and intrinsics checks, Staging and ProfScope.  Part of tcsfm_api.hip, the library's only translation unit: included
// after the kernels' headers and the plans (dense_plan.h, call_plan.h), before every *_host.h.
#pragma once
#include "device_owned.h"

namespace {

// (the tile geometry of the hot kernel and the layout constants: layout.h)

thread_local std::string g_create_error;

}  // namespace

// The scratch of the dense modes (dense_host.h), allocated by whichever mode first needs a buffer, at the handle's capacity for it
// (dense_plan.h: dense_caps): never re-sized while the handle lives, captured call graphs bake the pointers in.
struct DenseScratch {
    DevBuf<float> sel_maps;                            // dense window modes: the forward pairs' diff | valid maps, [2][max_pairs][H*W]
    DevBuf<float> dense_rec, depth0;                   // per-pixel records and prior centres of the pair-form dense kernels
    DevBuf<double> delta;                              // ... and their pose steps
    DevBuf<float> dense_rec2, depth_alt;               // ... second record / depth buffers of the fused back-substitution (ping-pong)
    DevBuf<float> dense_rec_acc, depth_acc;            // dense LM: accepted per-pixel records / depth maps
    DevBuf<int> lm_accept;
    // joint dense modes (one depth map per target shared by its S forward pairs): per-pixel records, workgroup records, per-target state
    DevBuf<float> jrec, jrec_acc, jblockrec, jdepth_acc;
    DevBuf<JointState> jstate;
    DevBuf<double> jdelta;
    DevBuf<double> jpart;                              // split record sums of the joint solve (JointSolveParams::nsplit): [2][8][NACC] fp64
    DevBuf<int> jtick;                                 // ... and their tickets, zero between launches
    // dense mode on the reference's loss (dense_ref_kernel.h): mask counts, fixed-point scatter sums, linearisation export
    DevBuf<int> dref_norms;
    DevBuf<long long> dref_ext;
    DevBuf<double> dref_export;
    DevBuf<float> dref_smooth;                         // l_smooth: [targets][2] mean of the sigmoid disparity, the target's whole term (k_dref_smooth)
    DevBuf<float> qres_rho, qres_rec;                  // TCSFM_DEPTH_QUARTER: [2][targets][H/4 * W/4] cell unknowns, [targets][cells][JREC] cell records
    // free source depth maps (opts.free_source_depths): the inverse pairs as groups of one source
    DevBuf<float> jrec_src;
    DevBuf<JointState> jstate_src;
    DevBuf<double> jdelta_src;
    DevBuf<long long> dref_ext_src;
    DevBuf<float> qres_rho_src, qres_rec_src;          // ... in the quarter-resolution parametrisation
};

// Ownership: every stream, event and device buffer below is an owner of device_owned.h and releases itself when the handle is deleted.
// Members are destroyed in reverse order of declaration, so THE STREAMS ARE DECLARED FIRST and everything that work on them may touch
// (events, buffers, the status word) after them: the buffers go before their streams do.  tcsfm_destroy deletes the handle only after it
// has synchronised every stream that work may be on.
struct tcsfm_ctx {
    int device = 0, H = 0, W = 0, max_pairs = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;      // where the calls run: own_stream, or the caller's (tcsfm_set_stream; not owned)
    Stream aux_stream;                 // joint dense mode: the inverse pairs' refinement runs beside the forward group's (fork / join by events)
    Stream seq_copy;                   // tcsfm_refine_sequence: the copy stream of the device ring of frames
    Stream seq_pack;                   // k_frame_pack runs here, behind the chunk's copy (event), beside the next chunk's copy
    Event aux_fork, aux_join;
    MappedWord err_word;               // host-mapped status word of the device-side guards
    DevBuf<float4> tgtpack, srcpack;
    DevBuf<float> depth_work;
    DevBuf<float> partials, blockrec;
    DevBuf<int> tickets;
    DevBuf<PairState> state;
    DevBuf<PairConst> pconst;
    DevBuf<double> lin_out;            // device [max_pairs][7*7+7+4]
    DevBuf<float> pose_dev, ls_dev, K_dev;
    int tiles_x = 0, tiles_y = 0, nblk = 0, ngrp = 0, ngrp_pad = 0, stats_cap_iters = 0;
    int nblk_alloc = 0, ngrp_alloc = 0;   // scratch capacity of the pose path and of the pair-form dense kernels (16 x 16 tiles or coarser)
    DenseScratch dense;                    // the dense modes' scratch, allocated on first use
    DenseCaps caps;                        // ... and every buffer's capacity (dense_plan.h), fixed at create
    // tcsfm_warp_backward (warp_grad_kernel.h), allocated on first use: workgroup records of the pose gradient [max_pairs][blocks][12],
    // fixed-point scatter sums [max_pairs][H*W], per-item max |g_proj_depth| (bit patterns)
    DevBuf<double> wgrad_rec;
    DevBuf<long long> wgrad_fix;
    DevBuf<unsigned> wgrad_gmax;
    // tcsfm_photometric_backward (photo_grad_kernel.h), allocated on first use: the warp's forward (img_rec | proj_depth | comp_depth) and
    // the cotangents that reach it (g_rec | g_proj_depth | g_comp_depth), each [max_pairs][5][H*W]
    DevBuf<float> pgrad_fwd, pgrad_cot;
    DevBuf<unsigned> scale_keys, scale_hist;   // scale recovery scratch (keys, 256 bins + 4 state words)
    DevBuf<long long> dbg_stamps;      // TCSFM_DEBUG_STAMPS=1: 8 wall-clock stamps of the last k_solve launch (100 MHz ticks)
    std::vector<DevBuf<char>> stage;    // device staging for host-pointer calls (Staging), in bytes
    std::string err;
    // lanes (tcsfm_set_lanes): lane k >= 1 is a child handle with its own stream and scratch, so that several refine calls are
    // in flight at once; lane 0 is this handle.  in_ev orders a lane behind the work queued on the parent's stream at call time,
    // done_ev is what tcsfm_lane_wait makes the parent's stream wait for.
    std::vector<tcsfm_ctx *> lanes;    // (handles of their own: tcsfm_destroy destroys them first)
    Event in_ev, done_ev;
    Events marks;                      // tcsfm_lane_event: a ring of events handed out to the caller
    size_t mark_next = 0;
    // tcsfm_refine_sequence: device ring of frames, per-slot / per-window events, pose staging (allocated on first use)
    DevBuf<float> seq_img, seq_depth;  // [slots][3][H][W] and [slots][H][W]: ring slots, then mirror slots
    DevBuf<float> seq_pose_in, seq_pose_out, seq_ls_out;      // [windows][pairs][6 | 6 | 1], per call in the window form's stacked order
    DevBuf<float> seq_K;               // one copy of K per window of a call
    DevBuf<float4> seq_fpack;          // frame-level pack cache of the ring: [slots][H+2][W+2] (rgb, depth) + [slots][H][W] depth planes,
    DevBuf<float> seq_fdepth;          // for as many slots as seq_depth holds
    DevBuf<int> pair_idx;              // [2][max_pairs] ring slots of every pair's source pack / target depth plane (k_pack_cached)
    DevBuf<float> seq_dense;           // tcsfm_refine_dense_sequence: refined depth maps of all windows, per-window order (the parent's only)
    DevBuf<float> seq_dense_tmp;       // ... this context's stacked maps of one call (every lane's, lane 0 included)
    Events seq_copied, seq_done, seq_raw;      // per chunk: frames usable by the lanes / per call: done / per chunk: raw frames landed
    tcsfm_depthnet *seq_dn = nullptr;  // tcsfm_sequence_depthnet: the network whose clone computes the ring's depths on seq_pack when a sequence
                                       // call gets depths == NULL (not owned; tcsfm_depthnet_destroy detaches it)
    int seq_fmt = TCSFM_FRAMES_F32_CHW;  // tcsfm_sequence_frame_format: how the sequence calls read their `frames` argument
    DevBuf<uint8_t> seq_u8;            // U8 formats: device ring of the frames' BYTES (R slots of 3 H W -- or, with a frame source set, of
                                       // 3 src_h src_w -- bytes, no mirror slots); k_frames_u8 / k_resize_u8 turns a chunk into the floats of seq_img on seq_pack
    int seq_src_h = 0, seq_src_w = 0;  // tcsfm_sequence_frame_source: the camera's frame size (0, 0: none -- frames arrive at H x W)
    struct OwnedResizeTable : ResizeTable { DevBuf<int> blob; };      // a table with the device copy its `dev` points at
    std::vector<OwnedResizeTable> resize_tabs; // coefficient tables of the source sizes seen so far (resize_table())
    // tcsfm_sequence_scale: the sequence calls' per-frame scale stage (k_ground + k_median_frames on seq_pack, once per chunk)
    float seq_cam_height = 0.f;        // > 0: the stage is on
    DevBuf<unsigned> seq_scale_keys;   // key planes of ONE chunk (not scale_keys: the operators on the handle's stream own that)
    DevBuf<float> seq_scale_dev;       // results by ABSOLUTE frame index: [n] scales | [n] medians | [n] counts (int32), n = cap / 3
    std::vector<float> seq_scale_res;  // the last call's results on the host, same layout with cap = seq_scale_T (counts as bit patterns)
    int seq_scale_T = 0;               // 0: nothing kept
    // tcsfm_sequence_disparity: the sequence calls' disparity stage (the depth stage's head / a second, mirrored pass + k_disp_post on seq_pack)
    int seq_disp_mode = TCSFM_SEQ_DISP_OFF;
    DevBuf<char> seq_disp_dev;         // every frame's plane by ABSOLUTE frame index: [T][H][W] float32 (PLAIN) or float64 (POST)
    int seq_disp_T = 0, seq_disp_kept = TCSFM_SEQ_DISP_OFF;      // the last call's T (0: nothing kept) and mode, for tcsfm_sequence_disparities
    DevBuf<double> flip_ramp;          // l_mask [W] of the flip post-processing on the device (flip_ramp_device), built on first use
    // tcsfm_sequence_depth_eval: one group of staged ground truth and the call's metrics, grown when a call needs more
    DevBuf<char> eval_gt_dev;          // (bytes)
    DevBuf<double> eval_out_dev;       // [frames][TCSFM_NEVAL]
    struct KOk { const float *p; int n; };
    KOk K_ok[4] = {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}, {nullptr, 0}};   // device intrinsics pointers (and counts) that already passed the pinhole check
    int K_ok_next = 0;
    // The routing of the refine calls (call_host.h), by the rules of call_plan.h:
    GraphCache<hipGraphExec_t> graphs; // tcsfm_set_graph_replay: repeated device-pointer refine calls (same arguments) replayed as ONE captured HIP graph
    bool capturing = false;            // ... a capture is under way on the handle's stream
    CallQueue<CallArgs> queue;         // the *_queued entries: calls of one shape waiting to run as ONE launch sequence (tcsfm_set_coalesce / tcsfm_flush)
    LaneRotation rot;                  // ... and the streams their merged sequences alternate over (tcsfm_set_coalesce_lanes)
    bool lanes_serial = false;         // tcsfm_set_lanes' self-probe found that this process's streams do NOT run side by side (they slow each other
                                       // down: include/tcsfm.h "lanes"): the *_async calls run on the handle's own stream, one after the other
    float lane_probe[2] = {0.f, 0.f};  // the probe's figures: ms of the stand-in launches on ONE stream / alternating over TWO streams
    bool dref_dirty = true;            // the scatter sums (dref_ext, dref_ext_src) may be non-zero: a call that ran to its end leaves them zero
                                       // (k_dense_joint clears what it consumes); a fresh allocation, an export or a failed call does not
    DevBuf<double> pose_lin;           // l_pose_consist: [2][max_pairs][12] transforms at the linearisation (k_solve, kernels.h)
    unsigned short *trace_bits = nullptr;   // tcsfm_debug_trace: caller-owned device buffers (null = off)
    int *trace_decide = nullptr;
    long long trace_bits_cap = 0, trace_decide_cap = 0;
    bool tickets_dirty = false;        // a failed call may have left group tickets non-zero
    // event profiling (tcsfm_profile_*): one (start, stop, class) triple per bracketed launch
    bool profiling = false;
    DevBuf<unsigned long long> stamp_buf;      // in-kernel workgroup stamps of the linearisation launches of a profile session
    size_t stamp_cap = 0, stamp_used = 0;      // capacity / use in (start, end) pairs
    std::vector<std::pair<size_t, size_t>> stamp_launch;   // (first pair, workgroups) of every stamped launch
    Events ev_pool;
    std::vector<int> ev_class;
    size_t ev_used = 0;
};

namespace {

// Every entry point runs on the handle's device and leaves the caller's current device as it found it (a process driving several
// GPUs from one thread keeps allocating on the device it selected).
struct DeviceGuard {
    int prev = -1, dev;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            (h)->tickets_dirty = true;                                                               \
            return TCSFM_E_HIP;                                                                      \
        }                                                                                            \
    } while (0)

// a buffer of the handle's (or of an object on it) at n elements or more, from this call site: returns TCSFM_E_HIP with h->err set when it cannot be had
#define RESERVE(h, buf, n) HIPCHK(h, DEV_RESERVE(buf, n))

int fail(tcsfm_ctx *h, int code, const char *msg) {
    h->err = msg;
    return code;
}

// the code of a create / load whose allocations stopped at `e`
int fail_alloc(tcsfm_ctx *h, hipError_t e, const char *msg) { return fail(h, e == hipErrorOutOfMemory ? TCSFM_E_NOMEM : TCSFM_E_HIP, msg); }

// a call's arrays against the overlap contract of include/tcsfm.h: TCSFM_E_ARG with "<entry>: <out> overlaps <other>", or TCSFM_OK
int check_overlap(tcsfm_ctx *h, const char *entry, const ArgRanges &a) {
    std::string msg;
    return a.refused(entry, msg) ? fail(h, TCSFM_E_ARG, msg.c_str()) : TCSFM_OK;
}

// The device-side pinhole guards (init_pair, k_ground) raise a host-mapped status word; it is reported -- as the documented
// TCSFM_E_INTRINSICS -- by the next call on the handle or by tcsfm_synchronize, without a device synchronisation of its own.
static bool k_known(const tcsfm_ctx *h, const float *K, int n) {
    for (const auto &k : h->K_ok) if (k.p == K && K && n <= k.n) return true;
    return false;
}
static void k_add(tcsfm_ctx *h, const float *K, int n) {
    for (auto &k : h->K_ok) if (k.p == K) { if (n > k.n) k.n = n; return; }
    h->K_ok[h->K_ok_next] = {K, n};
    h->K_ok_next = (h->K_ok_next + 1) % 4;
}
static void k_forget(tcsfm_ctx *h) { for (auto &k : h->K_ok) k = {nullptr, 0}; }

int pending_error(tcsfm_ctx *h) {
    volatile int *raised = h->err_word.host;
    if (raised && *raised) {
        *raised = 0;
        k_forget(h);
        return fail(h, TCSFM_E_INTRINSICS, "an earlier asynchronous call was given non-pinhole intrinsics (detected on the device): its results are NaN");
    }
    return TCSFM_OK;
}

int check_common(tcsfm_ctx *h, const tcsfm_opts *o, int N) {
    if (!h) return TCSFM_E_ARG;
    if (!o) return fail(h, TCSFM_E_ARG, "opts is NULL");
    if (N < 1 || N > h->max_pairs) return fail(h, TCSFM_E_ARG, "N out of range for this handle (1..max_pairs)");
    if (o->refine != TCSFM_REFINE_POSE && o->refine != TCSFM_REFINE_POSE_SCALE) return fail(h, TCSFM_E_ARG, "opts.refine unsupported");
    if (o->solver != TCSFM_SOLVER_GN && o->solver != TCSFM_SOLVER_LM) return fail(h, TCSFM_E_ARG, "opts.solver unsupported");
    if (o->param != TCSFM_PARAM_SE3 && o->param != TCSFM_PARAM_EULER) return fail(h, TCSFM_E_ARG, "opts.param unsupported");
    if (o->n_iters < 0 || o->n_iters > 1000) return fail(h, TCSFM_E_ARG, "opts.n_iters out of range");
    if (o->depth_is_disp && !(o->min_depth > 0 && o->max_depth > o->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    if (o->window_rule != TCSFM_WINDOW_PAIR && o->window_rule != TCSFM_WINDOW_REFERENCE) return fail(h, TCSFM_E_ARG, "opts.window_rule unsupported");
    if (!(o->w_pose_consist >= 0.f) || (o->w_pose_consist > 0.f && (o->window_rule != TCSFM_WINDOW_REFERENCE || o->solver != TCSFM_SOLVER_GN ||
                                                                   o->refine != TCSFM_REFINE_POSE || o->param != TCSFM_PARAM_SE3)))
        return fail(h, TCSFM_E_ARG, "opts.w_pose_consist needs window_rule = TCSFM_WINDOW_REFERENCE, the Gauss-Newton solver, TCSFM_REFINE_POSE and the SE(3) chart");
    return TCSFM_OK;
}

// The overlap contract (include/tcsfm.h) for the refine family, pose and dense modes, applied by every public form on its own behalf
// before anything else happens (a graph replay and a queued call never reach the bodies' own staging with the caller's pointers).  The
// arrays' extents are the call plan's (call_plan.h).
// Honoured: pose_out at pose_in, and the dense depth_out anywhere over depth_t / depth_s -- *depth_on_input then says so (device pointers).  Arguments the
// later validation refuses (NULL handle or options, sizes out of range) are left to it.
int refine_overlap(tcsfm_ctx *h, const char *entry, const tcsfm_opts *o, int N, int win_B, int win_S, const CallArgs &c, bool dense,
                   bool *depth_on_input = nullptr) {
    if (depth_on_input) *depth_on_input = false;
    if (!h || !o || N < 1 || N > h->max_pairs || o->n_iters < 0 || o->n_iters > 1000) return TCSFM_OK;
    const PosePlan pl = pose_plan(N, win_B, win_S, 0, 0, 0, o->solver, o->n_iters, o->refine, o->argmin);
    const size_t hw = (size_t)h->H * h->W, f = sizeof(float);
    const bool scale = !dense && pl.np == 7;
    ArgRanges a;
    a.io_free = o->host_ptrs != 0;
    a.in("tgt", c.tgt, pl.tgt(hw) * f); a.in(win_B ? "srcs" : "src", c.src, pl.src(hw) * f); a.in("depth_t", c.depth_t, pl.depth_t(hw) * f);
    a.in("depth_s", c.depth_s, pl.depth_s(hw) * f); a.in("K", c.K, pl.K() * f); a.in("pose_in", c.pose_in, pl.pose() * f);
    if (scale) a.in("log_scale_in", c.log_scale_in, pl.log_scale() * f);
    a.out("pose_out", c.pose_out, pl.pose() * f);
    if (scale) a.out("log_scale_out", c.log_scale_out, pl.log_scale() * f);
    if (dense) a.out("depth_out", c.depth_out, pl.maps(hw) * f);
    a.out("stats_out", c.stats_out, pl.stats() * f);
    a.bless("pose_out", "pose_in");
    if (dense) { a.bless_any("depth_out", "depth_t"); a.bless_any("depth_out", "depth_s"); }
    std::string msg;
    if (a.refused(entry, msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    // (staged host arrays land in the library's own, disjoint device buffers: nothing to avoid there)
    if (depth_on_input) *depth_on_input = dense && !a.io_free && (a.overlap("depth_out", "depth_t") || a.overlap("depth_out", "depth_s"));
    return TCSFM_OK;
}

// The array arguments of one call.  With opts.host_ptrs in() stages a host array on the device and out() hands out a device buffer
// that finish() copies back to its host pointer; with device pointers both pass the pointer through.  The device buffers are the
// handle's staging slots (grown on demand), taken in order of registration -- a null argument takes its slot too, so an argument's
// slot does not depend on which optional arguments a call passes.  Every array is registered under its argument's name with its
// extent: ready() applies the overlap contract of include/tcsfm.h (arg_overlap.h) -- a forbidden overlap refuses the call before
// anything is enqueued -- and only then sends the staged inputs up.  The first error sticks in rc: later steps do nothing.  Holds the
// handle's device for the call and starts with the pending device-side error check.
struct Staging {
    tcsfm_ctx *h;
    const tcsfm_opts *o;
    DeviceGuard dev_guard;
    int rc = TCSFM_OK;
    size_t slot = 0;
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<Back> back, up;
    ArgRanges args;

    Staging(tcsfm_ctx *h_, const tcsfm_opts *o_) : h(h_), o(o_), dev_guard(h_->device) {
        rc = pending_error(h);
        args.io_free = o->host_ptrs != 0;
    }

    // the next slot's device buffer, at least `bytes` long (null after an error)
    void *scratch(size_t bytes) {
        const size_t i = slot++;
        if (rc) return nullptr;
        if (h->stage.size() <= i) h->stage.resize(i + 1);
        rc = grow(h->stage[i], bytes);
        return rc ? nullptr : h->stage[i].p;
    }
    int grow(DevBuf<char> &b, size_t bytes) {
        RESERVE(h, b, bytes);
        return TCSFM_OK;
    }
    template <typename T>
    const T *in(const char *name, const T *p, size_t count) {
        args.in(name, p, count * sizeof(T));
        if (!o->host_ptrs || !p) { slot++; return p; }
        void *d = scratch(count * sizeof(T));
        if (d) up.push_back({const_cast<T *>(p), d, count * sizeof(T)});
        return (const T *)d;
    }
    template <typename T>
    T *out(const char *name, T *p, size_t count) {
        args.out(name, p, count * sizeof(T));
        if (!o->host_ptrs || !p) { slot++; return p; }
        void *d = scratch(count * sizeof(T));
        if (d) back.push_back({p, d, count * sizeof(T)});
        return (T *)d;
    }
    // an output that is written on the host in every mode (takes no slot)
    void host_out(const char *name, const void *p, size_t bytes) { args.out(name, p, bytes); }
    void bless(const char *out_name, const char *in_name) { args.bless(out_name, in_name); }
    // every array is registered: the overlap contract on behalf of `entry` (null: the caller has applied it), then the staged inputs go up
    int ready(const char *entry) {
        if (rc) return rc;
        std::string msg;
        if (entry && args.refused(entry, msg)) return rc = fail(h, TCSFM_E_ARG, msg.c_str());
        for (const Back &u : up)
            if ((rc = upload(const_cast<void *>(u.dev), u.host, u.bytes))) return rc;
        up.clear();
        return TCSFM_OK;
    }
    int upload(void *dev, const void *host, size_t bytes) {
        HIPCHK(h, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
        return TCSFM_OK;
    }
    // the outputs' copies back, in registration order, then a synchronisation when `sync` and the call staged host arrays
    int finish(bool sync = true) {
        if (rc) return rc;
        for (const Back &b : back) HIPCHK(h, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
        if (o->host_ptrs && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
        return TCSFM_OK;
    }
};

// intrinsics must be pinhole; checked on the host when they are host pointers, otherwise after a small D2H copy
int check_intrinsics(tcsfm_ctx *h, const tcsfm_opts *o, const float *K_host_or_dev, int n) {
    // Device intrinsics are validated with one blocking D2H copy the FIRST time a (pointer, count) is seen; repeated calls
    // on the same buffer (a sequence, the bench loop) stay fully asynchronous.  The device side guards independently:
    // init_pair() poisons the pose with NaN when K is not pinhole, so a buffer mutated behind our back still fails loudly.
    if (!o->host_ptrs && k_known(h, K_host_or_dev, n)) return TCSFM_OK;
    std::vector<float> k((size_t)n * 9);
    if (o->host_ptrs) memcpy(k.data(), K_host_or_dev, k.size() * sizeof(float));
    else {
        HIPCHK(h, hipMemcpyAsync(k.data(), K_host_or_dev, k.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    for (int i = 0; i < n; i++) {
        const float *K = &k[(size_t)i * 9];
        if (K[1] != 0.f || K[3] != 0.f || K[6] != 0.f || K[7] != 0.f || K[8] != 1.f || !(K[0] != 0.f) || !(K[4] != 0.f))
            return fail(h, TCSFM_E_INTRINSICS, "intrinsics must be pinhole [fx 0 cx; 0 fy cy; 0 0 1]");
    }
    if (!o->host_ptrs) k_add(h, K_host_or_dev, n);
    return TCSFM_OK;
}

// RAII bracket: records a start event now and a stop event at scope exit when profiling is on
struct ProfScope {
    tcsfm_ctx *h;
    bool on;
    ProfScope(tcsfm_ctx *h_, int cls) : h(h_), on(h_->profiling) {
        if (!on) return;
        if (h->ev_used + 2 > h->ev_pool.size()) {
            (void)h->ev_pool.grow(h->ev_pool.size() + 64, true);
            if (h->ev_used + 2 > h->ev_pool.size()) { on = false; return; }      // no event, no bracket
        }
        h->ev_class.push_back(cls);
        (void)hipEventRecord(h->ev_pool[h->ev_used], h->stream);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(h->ev_pool[h->ev_used + 1], h->stream);
        h->ev_used += 2;
    }
};

// while profiling, hand the next in-kernel stamp slots (one (start, end) pair per workgroup) to a linearisation launch
void take_stamp(tcsfm_ctx *h, LinParams &P, size_t workgroups) {
    P.stamp = nullptr;
    if (h->profiling && h->stamp_buf && h->stamp_used + workgroups <= h->stamp_cap) {
        P.stamp = h->stamp_buf + 2 * h->stamp_used;
        h->stamp_launch.emplace_back(h->stamp_used, workgroups);
        h->stamp_used += workgroups;
    }
}

}  // namespace
