// The plan of a pose call and the routing rules of the calls around it (pose_host.h, call_host.h), host only: what a pose call stages and
// launches, when queued calls run and which of them merge, which stream a merged sequence takes, and when a repeated call is captured
// and replayed.  Integer arithmetic and byte compares, no HIP, no environment, no handle: tests/asan/call_plan_host.cpp builds it alone and
// plays every rule against the invariants below over small alphabets.
//
// The invariants.
//  1. Pose plan.  The schedule of a call is n_iters x (LIN, solve mode 0) -- under Gauss-Newton the last of them emits the pose --, under
//     Levenberg-Marquardt followed by ONE (COST, solve mode 1) step that emits; n_iters == 0 has no step and finishes through k_finish.
//     n_lin, the figure the decision trace is sized by, is the number of steps: there is no second formula.
//  2. Pose plan.  tgt / K stand for nimg_t image sets and src for nimg_s: N / N for the pair form, B / B S for a window, and cB / cB cS --
//     ONE queued call's -- for a merged call, whose arrays come per call through the pointer table.  A window-form pack has a row per
//     FORWARD pair (N / 2), the pair form a row per pair.
//  3. Queue.  Every admitted call is launched exactly once, in admission order: a flush takes ALL waiting calls, and a call that cannot
//     join them (other kind, option bytes, B or S, or no room) flushes them first.
//  4. Queue.  The calls of one flush share kind, option bytes, B and S; there are at most max(1, coal_max) of them and their
//     2 B S n directed pairs fit max_pairs.
//  5. Queue.  A call that is not mergeable has run when its admission is complete, and nothing waits then.  Calls are left waiting only
//     while fewer than coal_max wait and one more of their shape still fits.
//  6. Queue.  A flush of an empty queue does nothing; every other flush is one batch of n calls in the counters.
//  7. Lanes.  Merged sequence k runs on lane k % nl, nl = 1 when the lanes run serially, else min(coal_lanes, lanes + 1).  Lane 0 is the
//     handle's own stream and never needs a join; a join visits every dirty lane once and leaves none dirty.
//  8. Graph cache.  It never holds more than `slots` entries; with slots == 0 it holds none and every call runs plainly.
//  9. Graph cache.  A call is captured only on an entry that was sighted before, has no executable, was never found uncapturable, and whose
//     intrinsics are known (a capture must not block on their validation).  A failed capture is never retried while the entry lives.
// 10. Graph cache.  A replay takes an entry whose key equals the call's byte for byte: any differing option byte, size or pointer misses.
// 11. Graph cache.  The entry evicted for a new one is the least recently used; every executable handed in comes back exactly once, from
//     an eviction or from drop_all(), for the caller to destroy.
#pragma once
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/tcsfm.h"
#include "layout.h"

namespace tc {

// ---- pose call plan
enum { POSE_STEP_COST = 0, POSE_STEP_LIN = 1 };      // a step's linearisation (kernels.h: MODE_COST, MODE_LIN)
struct PoseStep { int lin, it, solve_mode; bool emit; };      // emit: this solve writes the refined pose (and log-scale)

struct PosePlan {
    int N = 0, np = 6;                     // directed pairs; unknowns per pair (7: pose + log depth-scale)
    int nimg_t = 0, nimg_s = 0;            // image sets behind tgt (and K) / src
    int pack_rows = 0;                     // rows of workgroups of the pack launch
    int n_sel = 0;                         // forward pairs that take the per-pixel min over their window's sources (0: none)
    int n_iters = 0, n_lin = 0;            // n_lin: linearisation launches = steps of the schedule
    bool lm = false, window = false, finish = false;      // finish: nothing to solve, the pose goes round through k_finish

    // the schedule (invariant 1)
    PoseStep step(int i) const {
        if (i < n_iters) return {POSE_STEP_LIN, i, 0, !lm && i == n_iters - 1};
        return {POSE_STEP_COST, n_iters, 1, true};
    }
    // element extents of the array arguments at hw = H * W pixels
    size_t tgt(size_t hw) const { return (size_t)nimg_t * 3 * hw; }
    size_t src(size_t hw) const { return (size_t)nimg_s * 3 * hw; }
    size_t depth_t(size_t hw) const { return (size_t)nimg_t * hw; }
    size_t depth_s(size_t hw) const { return (size_t)nimg_s * hw; }
    size_t K() const { return (size_t)nimg_t * 9; }
    size_t pose() const { return (size_t)N * 6; }
    size_t log_scale() const { return (size_t)N; }
    size_t stats() const { return (size_t)N * (n_iters + 1) * TCSFM_NSTAT; }
    size_t maps(size_t hw) const { return (size_t)N * hw; }      // one map per directed pair (the dense modes' depth_out)
};

// linearisation launches of a call: one per iteration, and Levenberg-Marquardt's cost-only pass that decides on the last step
inline int pose_n_lin(int solver, int n_iters) { return n_iters + (solver == TCSFM_SOLVER_LM && n_iters > 0 ? 1 : 0); }

// N directed pairs; win_B x win_S: the window form (win_B == 0: the pair form); ncall > 0: ncall queued calls of cB x cS windows merged
// into this one (N = 2 cB cS ncall, win_B = cB ncall, win_S = cS).
inline PosePlan pose_plan(int N, int win_B, int win_S, int ncall, int cB, int cS, int solver, int n_iters, int refine, int argmin) {
    PosePlan p;
    p.N = N; p.np = refine == TCSFM_REFINE_POSE_SCALE ? 7 : 6;
    p.window = ncall > 0 || win_B > 0;
    p.nimg_t = ncall > 0 ? cB : (win_B ? win_B : N);
    p.nimg_s = ncall > 0 ? cB * cS : (win_B ? win_B * win_S : N);
    p.pack_rows = p.window ? N / 2 : N;
    p.n_sel = (win_B && win_S > 1 && argmin) ? win_B * win_S : 0;
    p.n_iters = n_iters; p.lm = solver == TCSFM_SOLVER_LM;
    p.n_lin = pose_n_lin(solver, n_iters);
    p.finish = n_iters == 0;
    return p;
}

// ---- which queued calls merge (include/tcsfm.h: tcsfm_set_coalesce).  trace_on: a decision trace is being recorded.
// The REFERENCE rule couples the windows of a pose call through its batch normalisers: such calls are never merged with others.
inline bool pose_mergeable(const tcsfm_opts &o, bool trace_on, int coal_max) {
    return coal_max > 1 && o.window_rule == TCSFM_WINDOW_PAIR && !trace_on;
}
// Dense calls: per-pair Gauss-Newton calls with ONE source per target, and the reference-loss mode with fixed source maps (every call is a
// normaliser group of its own inside the merged sequence).  A call whose depth_out lies on its own depth inputs is honoured by the path
// that writes depth_out last: it is not merged.
inline bool dense_mergeable(const tcsfm_opts &o, int S, int H, int W, bool trace_on, int coal_max, bool depth_on_input) {
    const bool plain = coal_max > 1 && o.solver == TCSFM_SOLVER_GN && o.n_iters >= 1 && o.param == TCSFM_PARAM_SE3 && !trace_on;
    const bool merge_ref = plain && o.window_rule == TCSFM_WINDOW_REFERENCE && S <= JMAXS && o.free_source_depths == 0 && o.prior_init >= 0.f && o.w_smooth >= 0.f &&
                           o.w_pose_consist == 0.f && (o.depth_param == TCSFM_DEPTH_FULL || (o.depth_param == TCSFM_DEPTH_QUARTER && H % 4 == 0 && W % 4 == 0)) &&
                           o.min_depth > 0 && o.max_depth > o.min_depth;
    return !depth_on_input && (merge_ref || (plain && S == 1 && o.window_rule == TCSFM_WINDOW_PAIR && o.w_dc == 0.f));
}

// The caller's arrays of one refine call, pose or dense (host or device pointers, as opts.host_ptrs says); null: not given / not wanted.
// The window forms pass their `srcs` as src; log_scale_*: pose + scale calls; depth_out: dense calls.
struct CallArgs {
    const float *tgt, *src, *depth_t, *depth_s, *K, *pose_in, *log_scale_in;
    float *pose_out, *log_scale_out, *depth_out, *stats_out;
};

// ---- call queue: calls of one kind, option block and shape waiting to run as ONE launch sequence.  admit() decides, push() / take() move
// the calls; the caller launches what take() hands back.
enum { CALL_POSE = 0, CALL_DENSE = 1 };
struct Admission { bool flush_before, enqueue, flush_after; };      // enqueue == false: the call runs directly, unqueued

template <class Call>
struct CallQueue {
    int kind = CALL_POSE, B = 0, S = 0;
    tcsfm_opts opts;
    std::vector<Call> waiting;
    int coal_max = 0, max_pairs = 0;
    int batches = 0, calls = 0;            // flushes so far and the calls they held (tcsfm_coalesce_counts)

    // n calls of B x S windows are 2 B S n directed pairs of one launch sequence
    bool fits(int B_, int S_, long long n) const { return (long long)2 * B_ * S_ * n <= max_pairs; }
    Admission admit(int kind_, const tcsfm_opts &o, int B_, int S_, bool mergeable) const {
        Admission a;
        if (kind_ == CALL_DENSE && !mergeable) {      // a dense call that cannot merge runs as the unqueued entry point does, behind what waits
            a.flush_before = !waiting.empty(); a.enqueue = false; a.flush_after = false;
            return a;
        }
        const bool joins = waiting.empty() || (kind == kind_ && memcmp(&opts, &o, sizeof(o)) == 0 && B == B_ && S == S_ && fits(B_, S_, (long long)waiting.size() + 1));
        const long long n = (joins ? (long long)waiting.size() : 0) + 1;      // calls waiting once this one is in
        a.flush_before = !joins; a.enqueue = true;
        a.flush_after = !mergeable || n >= coal_max || !fits(B_, S_, n + 1);
        return a;
    }
    void push(int kind_, const tcsfm_opts &o, int B_, int S_, const Call &c) {
        kind = kind_; opts = o; B = B_; S = S_;
        waiting.push_back(c);
    }
    // a flush: all waiting calls, counted as one batch; `seq` is the batch's number (lane rotation).  Empty queue: nothing, not counted.
    std::vector<Call> take(int *seq) {
        std::vector<Call> out;
        if (waiting.empty()) return out;
        out.swap(waiting);
        *seq = batches;
        batches++; calls += (int)out.size();
        return out;
    }
};

// ---- lane rotation of merged sequences (tcsfm_set_coalesce_lanes)
struct LaneRotation {
    int coal_lanes = 1;                    // merged sequences alternate over this many of the handle's streams
    unsigned dirty = 0;                    // bit l: lane l ran a merged sequence the handle's stream has not been ordered behind yet

    // lanes: the handle's lanes beside lane 0; serial: they do not run side by side (tcsfm_set_lanes' probe)
    int width(bool serial, int lanes) const { return serial ? 1 : std::min(coal_lanes, lanes + 1); }
    int lane_of(int seq, bool serial, int lanes) const {
        const int nl = width(serial, lanes);
        return nl > 1 ? seq % nl : 0;
    }
    void ran(int lane) { if (lane > 0) dirty |= 1u << lane; }
    // wait(l) orders the handle's stream behind lane l; its first non-zero result ends the join and leaves that lane dirty
    template <class Wait>
    int join(int lanes, Wait wait) {
        for (int l = 1; l <= lanes && dirty; l++)
            if (dirty & (1u << l)) {
                if (int rc = wait(l)) return rc;
                dirty &= ~(1u << l);
            }
        return 0;
    }
};

// ---- graph cache (tcsfm_set_graph_replay): which repeated call is captured, replayed, evicted.  Exec is the executable's handle;
// Exec() means none.
struct CallKey { tcsfm_opts o; int N, win_B, win_S, kind; const void *p[10]; };      // compared bytewise: make_key zeroes the padding
inline CallKey make_key(const tcsfm_opts &o, int kind, int N, int win_B, int win_S, const CallArgs &a) {
    CallKey k;
    memset(&k, 0, sizeof(k));
    k.o = o; k.N = N; k.win_B = win_B; k.win_S = win_S; k.kind = kind;
    const bool dense = kind == CALL_DENSE;      // a dense call takes no log-scales; its depth_out stands where a pose call's log_scale_out does
    const void *p[10] = {a.tgt, a.src, a.depth_t, a.depth_s, a.K, a.pose_in, dense ? nullptr : a.log_scale_in, a.pose_out,
                         dense ? (const void *)a.depth_out : (const void *)a.log_scale_out, a.stats_out};
    memcpy(k.p, p, sizeof(k.p));
    return k;
}

enum Sight {
    SIGHT_FIRST,       // not seen before: run plainly; the call is remembered (the plain run validates intrinsics and allocates scratch)
    SIGHT_PLAIN,       // run plainly: the cache is off, the entry is uncapturable, or its intrinsics would be validated again
    SIGHT_CAPTURE,     // capture the plain path's launches, then report captured() or uncapturable()
    SIGHT_REPLAY       // launch replay()'s executable
};

template <class Exec>
struct GraphCache {
    struct Entry { CallKey key; Exec exec; int seen; unsigned long long used; };      // seen: 1, or -1 once a capture failed
    int slots = 0;                         // 0: off
    std::vector<Entry> entries;
    unsigned long long clock = 0;
    int captures = 0, replays = 0;
    size_t cur = 0;                        // the entry of the last sight()

    // *evicted: the executable of the entry that made room on a first sighting (Exec(): none, or none to destroy)
    Sight sight(const CallKey &key, bool intrinsics_known, Exec *evicted) {
        *evicted = Exec();
        if (slots <= 0) return SIGHT_PLAIN;
        size_t i = 0;
        while (i < entries.size() && memcmp(&entries[i].key, &key, sizeof(key)) != 0) i++;
        cur = i;
        if (i == entries.size()) {
            if ((int)entries.size() >= slots) {      // evict the least recently used entry
                size_t lru = 0;
                for (size_t j = 1; j < entries.size(); j++) if (entries[j].used < entries[lru].used) lru = j;
                *evicted = entries[lru].exec;
                entries.erase(entries.begin() + lru);
            }
            cur = entries.size();
            entries.push_back({key, Exec(), 1, ++clock});
            return SIGHT_FIRST;
        }
        Entry &e = entries[i];
        if (e.exec != Exec()) return SIGHT_REPLAY;      // (replay() stamps the entry: the caller's own checks may still refuse the call)
        e.used = ++clock;
        return (e.seen != 1 || !intrinsics_known) ? SIGHT_PLAIN : SIGHT_CAPTURE;
    }
    Exec replay() { entries[cur].used = ++clock; return entries[cur].exec; }
    void replayed() { replays++; }
    void captured(Exec exec) { entries[cur].exec = exec; captures++; }
    void uncapturable() { entries[cur].seen = -1; }      // not capturable in this configuration: plain launches from now on
    std::vector<Exec> drop_all() {
        std::vector<Exec> out;
        for (const Entry &e : entries) if (e.exec != Exec()) out.push_back(e.exec);
        entries.clear();
        return out;
    }
};

}  // namespace tc
