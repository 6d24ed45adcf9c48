// The routing of the refine calls, pose and dense (include/tcsfm.h: tcsfm_set_graph_replay, tcsfm_set_coalesce and the *_queued entries,
// tcsfm_set_lanes and the *_async entries).  Every rule -- what is captured, replayed and evicted, when queued calls run and which of
// them merge, which lane a merged sequence takes -- is call_plan.h's (no HIP there); here is what is done about it: the capture, the
// events, the launches through pose_refine (pose_host.h) and dense_body.  Part of tcsfm_api.hip, the library's only translation unit:
// included after context.h, dense_host.h and dense_body, before the entry points.
#pragma once
#include "call_plan.h"

// Captured call graphs bake in the handle's scratch pointers and run on the stream they were last launched on: whoever frees or
// re-sizes such scratch, switches the stream or evicts an entry drains BOTH streams a replay can be on first.
static void sync_graph_streams(tcsfm_ctx *c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream && c->own_stream != c->stream) (void)hipStreamSynchronize(c->own_stream);
}
static void drop_graphs(tcsfm_ctx *c) {
    if (c->graphs.entries.empty()) return;
    sync_graph_streams(c);
    for (hipGraphExec_t exec : c->graphs.drop_all()) (void)hipGraphExecDestroy(exec);
}

// Graph replay (tcsfm_set_graph_replay).  A B = 1 refinement is nine short launches: ~42 us of host time against ~40 us of GPU time
// per call with three calls in flight -- on a slow host the launches, not the kernels, set the rate.  A call whose arguments (options,
// sizes, every pointer) equal those of an earlier call on this handle / lane is captured once (the second time it is seen: the first
// run validates the intrinsics and allocates scratch, which a capture must not) and replayed with ONE hipGraphLaunch from then on.
// The kernels, their order and their arguments are exactly those of the plain path (`body`): results are bit-identical.
// kind: CALL_POSE, or CALL_DENSE (the joint dense mode, which forks its inverse pairs onto a second stream when it runs plainly, keeps
// them on the captured stream: every graph is one chain of launches).
static int replay_graph(tcsfm_ctx *h, const tcsfm_opts *o, int kind, int N) {
    int rc = check_common(h, o, N);
    if (rc) return rc;
    DeviceGuard dev_guard(h->device);
    if ((rc = pending_error(h))) return rc;
    hipGraphExec_t exec = h->graphs.replay();
    if ((rc = clean_tickets(h))) return rc;                // (a failed call may have left group tickets non-zero: what the packs would do)
    if (kind == CALL_DENSE && (rc = dref_clean(h))) return rc;      // (what dense_ref_run does before its first launch)
    HIPCHK(h, hipGraphLaunch(exec, h->stream));
    h->graphs.replayed();
    return TCSFM_OK;
}
// the plain path's launches into a graph, then the graph's first launch; whatever does not capture runs plainly from now on
template <class Body>
static int capture_graph(tcsfm_ctx *h, Body body) {
    {
        DeviceGuard dev_guard(h->device);
        if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            h->graphs.uncapturable();
            return body();
        }
        h->capturing = true;
        const std::string err_before = h->err;
        int rc = body();
        h->capturing = false;
        hipGraph_t graph = nullptr;
        hipError_t ce = hipStreamEndCapture(h->stream, &graph);
        hipGraphExec_t exec = nullptr;
        if (rc == TCSFM_OK && ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            (void)hipGraphDestroy(graph);
            h->graphs.captured(exec);
            HIPCHK(h, hipGraphLaunch(exec, h->stream));
            return TCSFM_OK;
        }
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        h->graphs.uncapturable();
        h->err = err_before;
    }
    return body();
}
template <class Body>
static int replay_or_run(tcsfm_ctx *h, const tcsfm_opts *o, int kind, int N, int win_B, int win_S, const CallArgs &a, bool bypass, Body body) {
    const bool eligible = h && o && h->graphs.slots > 0 && !h->capturing && !o->host_ptrs && !bypass && !h->profiling && !h->trace_bits &&
                          !h->trace_decide && !h->dbg_stamps && h->stream != nullptr;
    if (!eligible) return body();
    hipGraphExec_t evicted = nullptr;
    // (intrinsics not yet validated: the plain run validates them with a blocking copy, which a capture must not hold)
    const Sight s = h->graphs.sight(make_key(*o, kind, N, win_B, win_S, a), k_known(h, a.K, win_B ? win_B : N), &evicted);
    if (evicted) { sync_graph_streams(h); (void)hipGraphExecDestroy(evicted); }      // (it may still be running)
    if (s == SIGHT_REPLAY) return replay_graph(h, o, kind, N);
    if (s == SIGHT_CAPTURE) return capture_graph(h, body);
    return body();
}

static int refine_impl(tcsfm_ctx *h, const tcsfm_opts *o, int N, int win_B, int win_S, const CallArgs &a, const WinOff *wo = nullptr,
                       const FrameCache *fc = nullptr) {
    return replay_or_run(h, o, CALL_POSE, N, win_B, win_S, a, wo != nullptr || fc != nullptr, [&]() { return pose_refine(h, o, N, win_B, win_S, a, wo, fc); });
}
static int dense_impl(tcsfm_ctx *h, const tcsfm_opts *o, int N, int win_B, int win_S, const CallArgs &a, const WinOff *wo = nullptr,
                      bool depth_on_input = false) {
    return replay_or_run(h, o, CALL_DENSE, N, win_B, win_S, a, wo != nullptr,
                         [&]() { return dense_body(h, o, N, win_B, win_S, a, wo, depth_on_input); });
}

// ---- lanes (tcsfm_set_lanes): lane 0 is the handle, lane k >= 1 a child handle with its own stream and scratch
static tcsfm_ctx *lane_of(tcsfm_ctx *h, int lane) {
    if (!h || lane < 0 || lane > (int)h->lanes.size()) return nullptr;
    return lane == 0 ? h : h->lanes[lane - 1];
}
// run() on lane c of h.  A lane starts behind everything queued on the parent's stream so far (the producers of the caller's device
// buffers) and marks its end for tcsfm_lane_wait / tcsfm_lane_synchronize and the join of the merged sequences; c == h: just run()
template <class Run>
static int on_lane(tcsfm_ctx *h, tcsfm_ctx *c, Run run) {
    if (c == h) return run();
    HIPCHK(h, hipEventRecord(c->in_ev, h->stream));
    HIPCHK(h, hipStreamWaitEvent(c->own_stream, c->in_ev, 0));
    c->stream = c->own_stream;
    if (int rc = run()) { h->err = c->err; return rc; }
    HIPCHK(h, hipEventRecord(c->done_ev, c->own_stream));
    return TCSFM_OK;
}

// ---- coalesced calls: queued B-window calls of one shape as ONE launch sequence (include/tcsfm.h)
// the handle's stream is ordered behind the merged sequences that ran on lanes (consumers queued on it see their poses)
static int join_coalesce_lanes(tcsfm_ctx *h) {
    return h->rot.join((int)h->lanes.size(), [&](int l) -> int {
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->lanes[l - 1]->done_ev, 0));
        return TCSFM_OK;
    });
}

// Every waiting call, as one batch.  Merged sequences alternate over the lanes of the rotation (tcsfm_set_coalesce_lanes): sequence k runs
// on its lane behind everything queued on the handle's stream so far; the short tail kernels of one sequence (k_solve: 20 workgroups,
// 6 us) then overlap the other's chip-filling launches.  tcsfm_flush / tcsfm_synchronize order the handle's stream behind them.
static int flush_pending(tcsfm_ctx *h) {
    int seq = 0;
    const std::vector<CallArgs> calls = h->queue.take(&seq);
    if (calls.empty()) return TCSFM_OK;
    const tcsfm_opts o = h->queue.opts;
    const int B = h->queue.B, S = h->queue.S, n = (int)calls.size(), N = 2 * B * S;
    const bool dense = h->queue.kind == CALL_DENSE;
    const int l = h->rot.lane_of(seq, h->lanes_serial, (int)h->lanes.size());
    tcsfm_ctx *c = lane_of(h, l);
    const int rc = on_lane(h, c, [&]() -> int {
        if (n == 1) return dense ? dense_impl(c, &o, N, B, S, calls[0]) : refine_impl(c, &o, N, B, S, calls[0]);
        const MergedCalls m(calls, B, S);
        CallArgs first = calls[0];          // the bodies' own checks and staging see the first call's arrays; the kernels read the tables
        first.log_scale_in = nullptr; first.log_scale_out = nullptr;
        return dense ? dense_body(c, &o, N * n, B * n, S, first, nullptr, false, &m) : pose_refine(c, &o, N * n, B * n, S, first, nullptr, nullptr, &m);
    });
    if (!rc) h->rot.ran(l);
    return rc;
}

// Calls noted by the *_queued entry points are launched -- and the handle's stream ordered behind the merged sequences that ran on lanes --
// before ANY other entry point puts work on the handle's stream, switches that stream or destroys the handle: a plain call never overtakes
// a call queued before it (producers and consumers of the caller's pose / depth buffers keep their program order; include/tcsfm.h).
static int drain_queued(tcsfm_ctx *h) {
    if (!h || (h->queue.waiting.empty() && !h->rot.dirty)) return TCSFM_OK;
    DeviceGuard dev_guard(h->device);
    if (int rc = flush_pending(h)) return rc;
    return join_coalesce_lanes(h);
}

int tcsfm_set_coalesce(tcsfm_handle h, int max_calls) {
    if (!h) return TCSFM_E_ARG;
    if (max_calls < 0 || max_calls > TC_MAX_COAL) return fail(h, TCSFM_E_ARG, "tcsfm_set_coalesce: 0 <= max_calls <= 16");
    int rc = flush_pending(h);
    h->queue.coal_max = max_calls;
    return rc;
}

int tcsfm_set_coalesce_lanes(tcsfm_handle h, int n_streams) {
    if (!h) return TCSFM_E_ARG;
    if (n_streams < 1 || n_streams > (int)h->lanes.size() + 1) return fail(h, TCSFM_E_ARG, "tcsfm_set_coalesce_lanes: 1 <= n_streams <= lanes of the handle (tcsfm_set_lanes)");
    DeviceGuard dev_guard(h->device);
    int rc = flush_pending(h);
    if (!rc) rc = join_coalesce_lanes(h);
    h->rot.coal_lanes = n_streams;
    return rc;
}

int tcsfm_flush(tcsfm_handle h) {
    if (!h) return TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    int rc = flush_pending(h);
    return rc ? rc : join_coalesce_lanes(h);
}

int tcsfm_coalesce_counts(tcsfm_handle h, int *batches, int *calls) {
    if (!h) return TCSFM_E_ARG;
    if (batches) *batches = h->queue.batches;
    if (calls) *calls = h->queue.calls;
    return TCSFM_OK;
}

// The one admission path of the three *_queued entries: the checks of a window call on device pointers, then what the queue's rule
// (call_plan.h: CallQueue::admit) says -- launch what waits, note the call or run it directly, launch again.  `name` heads the messages.
static int queued_call(tcsfm_ctx *h, int kind, const char *entry, const char *name, const tcsfm_opts *o, int B, int S, CallArgs a) {
    if (!h) return TCSFM_E_ARG;
    const bool dense = kind == CALL_DENSE;
    if (B < 1 || S < 1 || (long long)2 * B * S > h->max_pairs) return fail(h, TCSFM_E_ARG, (std::string(name) + ": need 1 <= 2*B*S <= max_pairs").c_str());
    int rc = check_common(h, o, 2 * B * S);
    if (rc) return rc;
    if (!a.tgt || !a.src || !a.depth_t || !a.depth_s || !a.K || !a.pose_in || !a.pose_out || (dense && !a.depth_out))
        return fail(h, TCSFM_E_ARG, (std::string(name) + ": NULL argument").c_str());
    if (o->host_ptrs) return fail(h, TCSFM_E_ARG, (std::string(name) + ": device pointers only").c_str());
    if (dense || o->refine != TCSFM_REFINE_POSE_SCALE) { a.log_scale_in = nullptr; a.log_scale_out = nullptr; }
    bool depth_on_input = false;
    if ((rc = refine_overlap(h, entry, o, 2 * B * S, B, S, a, dense, dense ? &depth_on_input : nullptr))) return rc;
    // (a profile session does not stop the merging: the merged launches are bracketed like any other -- bench.py's roofline.timed_mode)
    const bool trace_on = h->trace_bits || h->trace_decide;
    const bool mergeable = dense ? dense_mergeable(*o, S, h->H, h->W, trace_on, h->queue.coal_max, depth_on_input) : pose_mergeable(*o, trace_on, h->queue.coal_max);
    DeviceGuard dev_guard(h->device);
    const Admission ad = h->queue.admit(kind, *o, B, S, mergeable);
    if (ad.enqueue && (rc = check_intrinsics(h, o, a.K, B))) return rc;            // (blocking only the first time a pointer is seen)
    if (ad.flush_before && (rc = flush_pending(h))) return rc;
    if (!ad.enqueue) return tcsfm_refine_dense_window(h, o, B, S, a.tgt, a.src, a.depth_t, a.depth_s, a.K, a.pose_in, a.pose_out, a.depth_out, nullptr);
    h->queue.push(kind, *o, B, S, a);
    return ad.flush_after ? flush_pending(h) : TCSFM_OK;
}

int tcsfm_refine_window_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs, const float *depth_t,
                               const float *depth_s, const float *K, const float *pose_in, float *pose_out) {
    return queued_call(h, CALL_POSE, "tcsfm_refine_window_queued", "tcsfm_refine_window_queued", o, B, S,
                       CallArgs{tgt, srcs, depth_t, depth_s, K, pose_in, nullptr, pose_out, nullptr, nullptr, nullptr});
}

int tcsfm_refine_window_scale_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs, const float *depth_t,
                                     const float *depth_s, const float *K, const float *pose_in, const float *log_scale_in, float *pose_out,
                                     float *log_scale_out) {
    return queued_call(h, CALL_POSE, "tcsfm_refine_window_scale_queued", "tcsfm_refine_window_queued", o, B, S,
                       CallArgs{tgt, srcs, depth_t, depth_s, K, pose_in, log_scale_in, pose_out, log_scale_out, nullptr, nullptr});
}

// the dense counterpart: per-pair Gauss-Newton dense calls with ONE source per target and reference-loss calls with fixed source maps are
// merged (k_pack_coal, per-call pose and depth outputs through the pointer table); every other dense call runs at once, behind what waits
int tcsfm_refine_dense_window_queued(tcsfm_handle h, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs, const float *depth_t,
                                     const float *depth_s, const float *K, const float *pose_in, float *pose_out, float *depth_out) {
    return queued_call(h, CALL_DENSE, "tcsfm_refine_dense_window_queued", "tcsfm_refine_dense_window_queued", o, B, S,
                       CallArgs{tgt, srcs, depth_t, depth_s, K, pose_in, nullptr, pose_out, nullptr, depth_out, nullptr});
}

// ---- lane self-probe.  MEASURED HAZARD (round 4): how well the streams of a process run side by side depends on the order
// in which the process created them -- a handle created before the process's first device work gave four lanes that were SLOWER than one
// (10 k against 13.5 k frame-pairs/s; kernels of overlapping lanes 40-55 us instead of 11).  The mechanism inside the runtime was not
// identified, so the library measures the real thing: B = 1 refinements (the handle's own kernels, 4 Gauss-Newton iterations) on stand-in
// images, first one after the other on the handle's stream, then round-robin over all lanes -- a stand-in kernel on two streams does NOT
// show the state (it overlapped fine in a process whose four lanes ran at 0.72 of one: the first version of this probe).  Lanes that do
// not beat one stream are switched off: their calls run on the handle's own stream.  ~5 ms, once per tcsfm_set_lanes.
static int probe_lanes(tcsfm_ctx *h) {
    h->lanes_serial = false;
    h->lane_probe[0] = h->lane_probe[1] = 0.f;
    if (h->lanes.empty()) return TCSFM_OK;
    if (const char *e = getenv("TCSFM_LANE_PROBE")) { if (atoi(e) == 0) return TCSFM_OK; }
    const size_t hw = (size_t)h->H * h->W;
    const int L = (int)h->lanes.size() + 1;
    DevBuf<float> buf;                                          // tgt | src [3 H W each], depth_t | depth_s [H W each], K [9], pose in [12], pose out [L][12]
    const size_t nfl = 8 * hw + 9 + 12 + (size_t)L * 12;
    RESERVE(h, buf, nfl);
    float *tgt = buf, *src = buf + 3 * hw, *dt = buf + 6 * hw, *ds = buf + 7 * hw, *K = buf + 8 * hw, *pin = K + 9, *pout = pin + 12;
    {
        std::vector<float> img(8 * hw);
        for (size_t i = 0; i < 6 * hw; i++) { const size_t p = i % hw; img[i] = 0.5f + 0.25f * sinf(0.05f * (float)(p % h->W) + 0.3f * (float)(i / hw)) * cosf(0.07f * (float)(p / h->W)); }
        for (size_t i = 6 * hw; i < 8 * hw; i++) img[i] = 0.5f + 0.001f * (float)((i % hw) / h->W);
        const float Kh[9] = {0.58f * h->W, 0.f, 0.5f * h->W, 0.f, 1.9f * h->H, 0.5f * h->H, 0.f, 0.f, 1.f};
        const float ph[12] = {0.002f, -0.001f, -0.03f, 0.001f, -0.002f, 0.0005f, -0.002f, 0.001f, 0.03f, -0.001f, 0.002f, -0.0005f};
        HIPCHK(h, hipMemcpy(buf, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(K, Kh, sizeof(Kh), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(pin, ph, sizeof(ph), hipMemcpyHostToDevice));
    }
    tcsfm_opts o; tcsfm_default_opts(&o);
    struct OnOwnStream {                                        // the probe runs on the handle's own stream; every way out hands the caller's back
        tcsfm_ctx *h;
        hipStream_t keep;
        explicit OnOwnStream(tcsfm_ctx *h_) : h(h_), keep(h_->stream) { h->stream = h->own_stream; }
        ~OnOwnStream() { h->stream = keep; }
    } on_own_stream(h);
    int rc = TCSFM_OK;
    auto run = [&](int nl, int calls, float *ms) -> int {
        for (int pass = 0; pass < 2 && !rc; pass++) {           // (first pass: warm-up -- scratch allocations, intrinsics check)
            HIPCHK(h, hipDeviceSynchronize());
            const auto t0 = std::chrono::steady_clock::now();
            for (int k = 0; k < calls && !rc; k++)
                rc = tcsfm_refine_window_async(h, k % nl, &o, 1, 1, tgt, src, dt, ds, K, pin, nullptr, pout + (size_t)(k % nl) * 12, nullptr, nullptr);
            HIPCHK(h, hipDeviceSynchronize());
            *ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return rc;
    };
    const int calls = 24;
    if (h->max_pairs >= 2) {
        rc = run(1, calls, &h->lane_probe[0]);
        if (!rc) rc = run(L, calls, &h->lane_probe[1]);
    }
    k_forget(h);
    for (tcsfm_ctx *c : h->lanes) k_forget(c);
    if (rc) return rc;
    if (h->lane_probe[1] > 0.95f * h->lane_probe[0] && h->lane_probe[0] > 0.f) {
        h->lanes_serial = true;
        fprintf(stderr, "tcsfm: lanes do not overlap in this process (probe: %d B=1 refinements take %.0f us on one stream, %.0f us over %d lanes): lane "
                        "calls run on the handle's own stream; use the queued calls (tcsfm_set_coalesce) to keep the chip busy\n", calls,
                h->lane_probe[0] * 1e3, h->lane_probe[1] * 1e3, L);
    }
    return TCSFM_OK;
}

int tcsfm_lane_probe(tcsfm_handle h, int *serial, float *one_stream_ms, float *two_streams_ms) {
    if (!h) return TCSFM_E_ARG;
    if (serial) *serial = h->lanes_serial ? 1 : 0;
    if (one_stream_ms) *one_stream_ms = h->lane_probe[0];
    if (two_streams_ms) *two_streams_ms = h->lane_probe[1];
    return TCSFM_OK;
}

int tcsfm_set_lanes(tcsfm_handle h, int n_lanes) {
    if (!h) return TCSFM_E_ARG;
    if (n_lanes < 1 || n_lanes > 8) return fail(h, TCSFM_E_ARG, "tcsfm_set_lanes: 1 <= n_lanes <= 8");
    DeviceGuard dev_guard(h->device);
    if (int rc_ = flush_pending(h)) return rc_;
    if (int rc_ = join_coalesce_lanes(h)) return rc_;
    if ((int)h->lanes.size() + 1 > n_lanes) HIPCHK(h, hipStreamSynchronize(h->stream));     // (a lane about to go may still run a merged sequence)
    while ((int)h->lanes.size() + 1 > n_lanes) { tcsfm_destroy(h->lanes.back()); h->lanes.pop_back(); }
    h->rot.coal_lanes = std::min(h->rot.coal_lanes, n_lanes);
    while ((int)h->lanes.size() + 1 < n_lanes) {
        tcsfm_ctx *c = nullptr;
        int rc = tcsfm_create(&c, h->device, h->H, h->W, h->max_pairs);
        if (rc) return fail(h, rc, "tcsfm_set_lanes: could not create a lane");
        hipError_t e = c->in_ev.create();
        if (e == hipSuccess) e = c->done_ev.create();
        if (e != hipSuccess) { tcsfm_destroy(c); return fail(h, TCSFM_E_HIP, "tcsfm_set_lanes: hipEventCreate failed"); }
        c->graphs.slots = h->graphs.slots;
        h->lanes.push_back(c);
    }
    return probe_lanes(h);
}

int tcsfm_set_graph_replay(tcsfm_handle h, int max_graphs) {
    if (!h) return TCSFM_E_ARG;
    if (max_graphs < 0 || max_graphs > 64) return fail(h, TCSFM_E_ARG, "tcsfm_set_graph_replay: 0 <= max_graphs <= 64");
    DeviceGuard dev_guard(h->device);
    h->graphs.slots = max_graphs;
    if ((int)h->graphs.entries.size() > max_graphs) drop_graphs(h);
    for (tcsfm_ctx *c : h->lanes) { c->graphs.slots = max_graphs; if ((int)c->graphs.entries.size() > max_graphs) drop_graphs(c); }
    return TCSFM_OK;
}

int tcsfm_graph_replay_counts(tcsfm_handle h, int *captures, int *replays) {
    if (!h) return TCSFM_E_ARG;
    int c_ = h->graphs.captures, r_ = h->graphs.replays;
    for (tcsfm_ctx *c : h->lanes) { c_ += c->graphs.captures; r_ += c->graphs.replays; }
    if (captures) *captures = c_;
    if (replays) *replays = r_;
    return TCSFM_OK;
}

// The *_async entries: the unqueued window call on lane `lane` of the handle (lane 0, or lanes that do not run side by side: the handle itself)
template <class Run>
static int async_call(tcsfm_ctx *h, int lane, const char *entry, const tcsfm_opts *o, int B, int S, const CallArgs &a, bool dense, Run run) {
    if (int rc_q = drain_queued(h)) return rc_q;
    tcsfm_ctx *c = lane_of(h, lane);
    if (!c) return h ? fail(h, TCSFM_E_ARG, (std::string(entry) + ": no such lane (tcsfm_set_lanes)").c_str()) : TCSFM_E_ARG;
    if (o && o->host_ptrs == 1) return fail(h, TCSFM_E_ARG, (std::string(entry) + ": host_ptrs must be 0 (device) or 2 (pinned host, asynchronous)").c_str());
    if (B >= 1 && S >= 1 && (long long)2 * B * S <= h->max_pairs)
        if (int rc_a = refine_overlap(h, entry, o, 2 * B * S, B, S, a, dense)) return rc_a;
    if (c == h || h->lanes_serial) return run(h);
    DeviceGuard dev_guard(h->device);
    return on_lane(h, c, [&]() { return run(c); });
}

int tcsfm_refine_window_async(tcsfm_handle h, int lane, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                              const float *depth_t, const float *depth_s, const float *K, const float *pose_in,
                              const float *log_scale_in, float *pose_out, float *log_scale_out, float *stats_out) {
    return async_call(h, lane, "tcsfm_refine_window_async", o, B, S, CallArgs{tgt, srcs, depth_t, depth_s, K, pose_in, log_scale_in, pose_out, log_scale_out, nullptr, stats_out}, false,
                      [&](tcsfm_ctx *c) { return tcsfm_refine_window(c, o, B, S, tgt, srcs, depth_t, depth_s, K, pose_in, log_scale_in, pose_out, log_scale_out, stats_out); });
}

int tcsfm_refine_dense_window_async(tcsfm_handle h, int lane, const tcsfm_opts *o, int B, int S, const float *tgt, const float *srcs,
                                    const float *depth_t, const float *depth_s, const float *K, const float *pose_in, float *pose_out,
                                    float *depth_out, float *stats_out) {
    return async_call(h, lane, "tcsfm_refine_dense_window_async", o, B, S, CallArgs{tgt, srcs, depth_t, depth_s, K, pose_in, nullptr, pose_out, nullptr, depth_out, stats_out}, true,
                      [&](tcsfm_ctx *c) { return tcsfm_refine_dense_window(c, o, B, S, tgt, srcs, depth_t, depth_s, K, pose_in, pose_out, depth_out, stats_out); });
}
