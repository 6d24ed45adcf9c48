// Stand-alone sanitizer program for the plan of a pose call and the routing rules of the refine calls (csrc/call_plan.h).  Its own main,
// no Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I tightly_coupled_sfm_amd/csrc tests/asan/call_plan_host.cpp -o call_plan_host && ./call_plan_host
//
// (the runtimes are linked statically: the program then runs as it is wherever the process's library list does not start with them)
// It plays every rule of the header against the invariants at its top, over small alphabets.
//   Queue: every script of up to 6 calls over kind x two option blocks x three shapes x mergeable, for every coal_max and max_pairs of the
//     grid.  What a script does from a point on depends on what waits there and on nothing else (every check below is made on the calls of
//     the step itself), so scripts that arrive at the same waiting calls with the same number of calls to go are played ONCE from there:
//     all of them are covered, and the program counts how many that is.
//   Lane rotation: every (lanes, coal_lanes, serial).
//   Graph cache: every script of up to 8 sightings over 4 keys x capture outcome (drawn per sighting: a script may fail on one key and
//     succeed on another), for every slots and one of three ways the intrinsics become known, against a model written from the rules (a recency list, no clock); every executable handed in is counted out again.
//     Scripts that arrive at the same cache contents at the same position are played once from there, as for the queue.
//   Pose plan: both solvers at 0..5 iterations against the rules, and a hand-made table of extents.
#include <stdio.h>
#include <string.h>
#include <map>
#include <tuple>
#include <vector>
#include "call_plan.h"

using namespace tc;

static int bad = 0;
#define CHECK(cond, ...)                                                                             \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (bad++ < 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                            \
    } while (0)

static tcsfm_opts opts_block(int which) {
    tcsfm_opts o;
    memset(&o, 0, sizeof(o));
    o.n_iters = 4 + which; o.w_l1 = 0.15f; o.w_ssim = 0.85f; o.irls_eps = 1e-3f; o.min_depth = 0.06f; o.max_depth = 2.67f;
    return o;
}

// ---- queue -----------------------------------------------------------------------------------------------------------------------------
struct Sym { int kind, opt, B, S, merge; };
struct Noted { int id; Sym s; };              // what the driver keeps per waiting call
static const int kShapes[3][2] = {{1, 1}, {1, 2}, {2, 1}};

struct QueuePlayer {
    CallQueue<Noted> q;
    int admitted = 0, launched = 0;           // calls are numbered in admission order; `launched` of them have run, in that order

    void flush() {
        const int b0 = q.batches, c0 = q.calls;
        const bool was_empty = q.waiting.empty();
        int seq = -1;
        const std::vector<Noted> batch = q.take(&seq);
        if (was_empty) {                      // invariant 6
            CHECK(batch.empty() && q.batches == b0 && q.calls == c0 && seq == -1, "a flush of an empty queue does something");
            return;
        }
        const int n = (int)batch.size();
        CHECK(n >= 1 && seq == b0 && q.batches == b0 + 1 && q.calls == c0 + n && q.waiting.empty(), "counters: n %d seq %d", n, seq);
        CHECK(n <= std::max(1, q.coal_max), "a flush of %d calls at coal_max %d", n, q.coal_max);
        CHECK(2 * batch[0].s.B * batch[0].s.S * n <= q.max_pairs, "a flush of %d calls of %d x %d at max_pairs %d", n, batch[0].s.B, batch[0].s.S, q.max_pairs);
        for (const Noted &c : batch) {
            CHECK(c.id == launched, "call %d launched where %d was due", c.id, launched);      // invariant 3
            launched++;
            CHECK(c.s.kind == batch[0].s.kind && c.s.opt == batch[0].s.opt && c.s.B == batch[0].s.B && c.s.S == batch[0].s.S, "a flush mixes shapes");      // invariant 4
            CHECK(q.kind == c.s.kind && q.B == c.s.B && q.S == c.s.S, "the queue's shape is not its calls'");
            const tcsfm_opts o = opts_block(c.s.opt);
            CHECK(memcmp(&q.opts, &o, sizeof(o)) == 0, "the queue's options are not its calls'");
        }
    }
    // one *_queued call, as call_host.h routes it
    void call(const Sym &s) {
        const tcsfm_opts o = opts_block(s.opt);
        const Admission ad = q.admit(s.kind, o, s.B, s.S, s.merge != 0);
        if (ad.flush_before) flush();
        const int id = admitted++;
        if (!ad.enqueue) {                    // runs directly, unqueued
            CHECK(s.kind == CALL_DENSE && !s.merge, "only a dense call that cannot merge runs unqueued");
            CHECK(q.waiting.empty() && id == launched, "a direct call overtakes what waits");
            launched++;
            CHECK(!ad.flush_after, "flush after a direct call");
        } else {
            q.push(s.kind, o, s.B, s.S, Noted{id, s});
            if (ad.flush_after) flush();
        }
        if (!s.merge) CHECK(launched == admitted && q.waiting.empty(), "a call that cannot merge has not run when its admission is over");      // invariant 5
        if (!q.waiting.empty()) {
            CHECK((int)q.waiting.size() < q.coal_max, "%d calls left waiting at coal_max %d", (int)q.waiting.size(), q.coal_max);
            CHECK((long long)2 * q.B * q.S * ((long long)q.waiting.size() + 1) <= q.max_pairs, "calls left waiting although no further one fits");
        }
        CHECK(launched + (int)q.waiting.size() == admitted, "calls lost: %d launched, %d waiting, %d admitted", launched, (int)q.waiting.size(), admitted);
    }
};

static std::vector<Sym> alphabet(int max_pairs) {
    std::vector<Sym> a;
    for (int kind : {CALL_POSE, CALL_DENSE}) for (int opt : {0, 1}) for (auto &sh : kShapes) for (int merge : {0, 1})
        if (2 * sh[0] * sh[1] <= max_pairs) a.push_back({kind, opt, sh[0], sh[1], merge});      // (the entry points refuse the others before admit)
    return a;
}

typedef std::tuple<int, int, int, int, int, int> QState;      // calls to go, then what waits: kind, option block, B, S, how many
static std::map<QState, double> q_seen;
static long q_played = 0;
// plays every script of `left` further calls from p; returns how many scripts that is (each ends with the caller's tcsfm_flush)
static double play_queue(const QueuePlayer &p, const std::vector<Sym> &alpha, int left) {
    const bool idle = p.q.waiting.empty();
    const QState key(left, idle ? -1 : p.q.kind, idle ? -1 : p.q.waiting[0].s.opt, idle ? -1 : p.q.B, idle ? -1 : p.q.S, (int)p.q.waiting.size());
    auto it = q_seen.find(key);
    if (it != q_seen.end()) return it->second;
    q_played++;
    {
        QueuePlayer e = p;                    // the script ends here: tcsfm_flush launches what waits, a second one finds nothing
        e.flush();
        CHECK(e.launched == e.admitted && e.q.waiting.empty(), "calls still waiting after the last flush");
        e.flush();
    }
    double scripts = 1;
    if (left > 0)
        for (const Sym &s : alpha) {
            QueuePlayer n = p;
            n.call(s);
            scripts += play_queue(n, alpha, left - 1);
        }
    q_seen[key] = scripts;
    return scripts;
}

static double check_queue() {
    double scripts = 0;
    for (int coal_max : {0, 1, 2, 3, 16})
        for (int max_pairs : {2, 4, 8, 64}) {
            q_seen.clear();
            QueuePlayer p;
            p.q.coal_max = coal_max; p.q.max_pairs = max_pairs;
            scripts += play_queue(p, alphabet(max_pairs), 6);
        }
    // the two predicates, by hand: what merges is what include/tcsfm.h says merges
    tcsfm_opts o = opts_block(0);
    o.solver = TCSFM_SOLVER_GN; o.param = TCSFM_PARAM_SE3; o.window_rule = TCSFM_WINDOW_PAIR; o.depth_param = TCSFM_DEPTH_FULL;
    CHECK(pose_mergeable(o, false, 2) && !pose_mergeable(o, false, 1) && !pose_mergeable(o, false, 0) && !pose_mergeable(o, true, 16), "pose_mergeable");
    CHECK(dense_mergeable(o, 1, 17, 33, false, 2, false) && !dense_mergeable(o, 2, 17, 33, false, 2, false) && !dense_mergeable(o, 1, 17, 33, false, 2, true) &&
          !dense_mergeable(o, 1, 17, 33, true, 2, false) && !dense_mergeable(o, 1, 17, 33, false, 1, false), "dense_mergeable, pair rule");
    tcsfm_opts r = o;
    r.window_rule = TCSFM_WINDOW_REFERENCE;
    CHECK(!pose_mergeable(r, false, 16), "the REFERENCE rule couples a pose call's windows: never merged");
    CHECK(dense_mergeable(r, 4, 17, 33, false, 2, false) && !dense_mergeable(r, 5, 17, 33, false, 2, false), "dense_mergeable, reference loss: S <= 4");
    r.depth_param = TCSFM_DEPTH_QUARTER;
    CHECK(!dense_mergeable(r, 2, 17, 33, false, 2, false) && dense_mergeable(r, 2, 16, 32, false, 2, false), "dense_mergeable, quarter resolution: H, W multiples of 4");
    r.free_source_depths = 1;
    CHECK(!dense_mergeable(r, 2, 16, 32, false, 2, false), "dense_mergeable: free source maps are not merged");
    tcsfm_opts l = o;
    l.solver = TCSFM_SOLVER_LM;
    CHECK(!dense_mergeable(l, 1, 17, 33, false, 2, false), "dense_mergeable: Gauss-Newton only");
    l = o; l.w_dc = 0.1f;
    CHECK(!dense_mergeable(l, 1, 17, 33, false, 2, false), "dense_mergeable: the pair rule takes no w_dc");
    return scripts;
}

// ---- lane rotation ---------------------------------------------------------------------------------------------------------------------
static long check_lanes() {
    long cases = 0;
    for (int lanes = 0; lanes <= 7; lanes++)
        for (int coal_lanes = 1; coal_lanes <= lanes + 1; coal_lanes++)
            for (int serial = 0; serial <= 1; serial++) {
                LaneRotation r;
                r.coal_lanes = coal_lanes;
                const int nl = serial ? 1 : (coal_lanes < lanes + 1 ? coal_lanes : lanes + 1);
                unsigned expect = 0;
                for (int k = 0; k < 3 * 8 + 1; k++) {
                    const int l = r.lane_of(k, serial != 0, lanes);
                    CHECK(l == k % nl && l >= 0 && l <= lanes, "sequence %d on lane %d, nl %d", k, l, nl);
                    r.ran(l);
                    if (l) expect |= 1u << l;
                    CHECK(r.dirty == expect && !(r.dirty & 1u), "dirty mask %x, expected %x", r.dirty, expect);
                    if (k % 5 == 4 || k == 24) {      // a join now and then: every dirty lane once, none left
                        LaneRotation f = r;           // ... and one whose first wait fails: that lane stays dirty, the join ends there
                        int tried = 0;
                        const int rc = f.join(lanes, [&](int) { tried++; return 7; });
                        CHECK(expect ? (rc == 7 && tried == 1 && f.dirty == expect) : (rc == 0 && tried == 0), "a failed join");
                        unsigned visited = 0;
                        int visits = 0;
                        CHECK(r.join(lanes, [&](int l2) { visited |= 1u << l2; visits++; return 0; }) == 0, "join");
                        CHECK(visited == expect && visits == __builtin_popcount(expect) && r.dirty == 0, "join visited %x of %x", visited, expect);
                        expect = 0;
                    }
                    cases++;
                }
            }
    return cases;
}

// ---- graph cache -----------------------------------------------------------------------------------------------------------------------
static float g_arrays[16];
static CallArgs base_args() { return CallArgs{g_arrays, g_arrays + 1, g_arrays + 2, g_arrays + 3, g_arrays + 4, g_arrays + 5, g_arrays + 6, g_arrays + 7, g_arrays + 8, g_arrays + 9, g_arrays + 10}; }
static CallKey make_key_no(int k) {          // four keys: two differ in a pointer, one in a size, one in an option
    CallArgs a = base_args();
    tcsfm_opts o = opts_block(0);
    int N = 2;
    if (k == 1) a.pose_out = g_arrays + 11;
    if (k == 2) N = 4;
    if (k == 3) o.n_iters = 5;
    return make_key(o, CALL_POSE, N, 1, 1, a);
}

static const CallKey &key_no(int k) {
    static const CallKey keys[4] = {make_key_no(0), make_key_no(1), make_key_no(2), make_key_no(3)};
    return keys[k];
}

struct ModelEntry { int key, exec; bool failed; };      // exec: 0 none
struct GraphPlayer {
    GraphCache<int> c;
    std::vector<ModelEntry> model;           // most recently used LAST
    int next_exec = 1;
    unsigned long long out = 0;              // executables the cache holds (bit e: executable e; a script hands in 8 at the most)
    long handed_in = 0, handed_back = 0;

    void back(int exec) {
        CHECK(exec > 0 && exec < 64 && (out >> exec & 1), "executable %d handed back but not held (twice, or never handed in)", exec);
        out &= ~(1ull << exec);
        handed_back++;
    }
    bool sighting(int k, bool known, bool capture_succeeds) {      // -> this sighting was a capture
        const CallKey &key = key_no(k);
        int evicted = 0;
        const Sight s = c.sight(key, known, &evicted);
        size_t m = 0;
        while (m < model.size() && model[m].key != k) m++;
        if (c.slots == 0) {                   // invariant 8
            CHECK(s == SIGHT_PLAIN && c.entries.empty() && evicted == 0, "a cache without slots keeps something");
            return false;
        }
        if (m == model.size()) {              // not held: first sighting, the least recently used entry makes room
            CHECK(s == SIGHT_FIRST, "an unknown key is not a first sighting");
            if ((int)model.size() >= c.slots) {
                CHECK(evicted == model[0].exec, "evicted executable %d, least recently used entry holds %d", evicted, model[0].exec);      // invariant 11
                model.erase(model.begin());
            } else CHECK(evicted == 0, "eviction with room left");
            if (evicted) back(evicted);
            model.push_back({k, 0, false});
        } else {
            CHECK(evicted == 0, "eviction on a held key");
            ModelEntry e = model[m];
            model.erase(model.begin() + m);
            if (e.exec) {                     // invariant 10
                CHECK(s == SIGHT_REPLAY, "a captured call is not replayed");
                if (s == SIGHT_REPLAY) {
                    CHECK(c.replay() == e.exec && memcmp(&c.entries[c.cur].key, &key, sizeof(key)) == 0, "replay of another call's executable");
                    c.replayed();
                }
            } else if (!e.failed && known) {  // invariant 9: sighted before, no executable, never failed, intrinsics known
                CHECK(s == SIGHT_CAPTURE, "a capturable call is not captured");
                if (s == SIGHT_CAPTURE) {
                    if (capture_succeeds) { e.exec = next_exec++; c.captured(e.exec); out |= 1ull << e.exec; handed_in++; }
                    else { e.failed = true; c.uncapturable(); }
                }
            } else CHECK(s == SIGHT_PLAIN, "capture of an entry that %s", e.failed ? "failed before" : "has unknown intrinsics");
            model.push_back(e);
        }
        CHECK(s != SIGHT_CAPTURE || known, "capture without known intrinsics");
        // the cache holds the model's keys, no more than `slots`
        CHECK((int)c.entries.size() <= c.slots && c.entries.size() == model.size(), "%d entries, %d slots, model %d", (int)c.entries.size(), c.slots, (int)model.size());
        for (const ModelEntry &e : model) {
            const CallKey &mk = key_no(e.key);
            size_t i = 0;
            while (i < c.entries.size() && memcmp(&c.entries[i].key, &mk, sizeof(mk)) != 0) i++;
            CHECK(i < c.entries.size() && c.entries[i].exec == e.exec && (c.entries[i].seen == -1) == e.failed, "the cache does not hold key %d as the model does", e.key);
        }
        return s == SIGHT_CAPTURE;
    }
    void end() {                              // drop_all: every executable still held, once
        for (int exec : c.drop_all()) back(exec);
        CHECK(out == 0 && c.entries.empty() && handed_in == handed_back, "%ld executables handed in, %ld handed back", handed_in, handed_back);
    }
};

// As for the queue: what a script does from a point on depends on the position and on what the cache holds -- per entry, in the cache's own
// order: which key, whether with an executable, whether found uncapturable, and its rank by last use -- so scripts that arrive there alike
// are played once from there.  (Which executable an entry holds does not matter: the model tells them apart, the cache only hands them on.)
static std::map<unsigned long long, double> g_seen;
static long g_played = 0;
static double play_graph(const GraphPlayer &p, int pos, int known_mode) {
    unsigned long long key = (unsigned long long)pos + 1;      // position, then 3 + 1 + 1 + 3 bits per entry
    for (const auto &e : p.c.entries) {
        unsigned rank = 0, k = 0;
        for (const auto &f : p.c.entries) rank += f.used < e.used ? 1 : 0;
        while (k < 4) { const CallKey &ck = key_no(k); if (!memcmp(&ck, &e.key, sizeof(ck))) break; k++; }
        key = (key << 8) | (k << 5) | ((e.exec != 0) << 4) | ((e.seen == -1) << 3) | rank;
    }
    auto it = g_seen.find(key);
    if (it != g_seen.end()) return it->second;
    g_played++;
    {
        GraphPlayer e = p;
        e.end();
    }
    double scripts = 1;
    if (pos < 8)
        for (int k = 0; k < 4; k++)
            for (int succeeds = 1; succeeds >= 0; succeeds--) {      // the outcome of a capture is drawn per sighting -- where the sighting is one
                GraphPlayer n = p;
                // intrinsics known: never / always / from the script's fourth sighting on (the plain runs before validated them)
                const bool captured = n.sighting(k, known_mode == 1 || (known_mode == 2 && pos >= 3), succeeds != 0);
                scripts += play_graph(n, pos + 1, known_mode);
                if (!captured) break;
            }
    g_seen[key] = scripts;
    return scripts;
}

static double check_graphs() {
    double scripts = 0;
    for (int slots : {0, 1, 2, 4})
        for (int known_mode = 0; known_mode < 3; known_mode++) {
            g_seen.clear();
            GraphPlayer p;
            p.c.slots = slots;
            scripts += play_graph(p, 0, known_mode);
        }
    // a key that differs in any single field misses (invariant 10): one captured call, then its neighbours, in a cache with room for all
    GraphCache<int> c;
    c.slots = 1024;
    const tcsfm_opts o = opts_block(0);
    const CallArgs a = base_args();
    int ev = 0;
    for (int kind : {CALL_POSE, CALL_DENSE}) {
        const CallKey k0 = make_key(o, kind, 2, 1, 1, a);
        CHECK(c.sight(k0, true, &ev) == SIGHT_FIRST && c.sight(k0, true, &ev) == SIGHT_CAPTURE, "the base call is not captured");
        c.captured(100 + kind);
        CHECK(c.sight(k0, true, &ev) == SIGHT_REPLAY && c.replay() == 100 + kind, "the base call is not replayed");
        int misses = 0;
        auto miss = [&](const CallKey &k, const char *what) { CHECK(c.sight(k, true, &ev) == SIGHT_FIRST && ev == 0, "a key that differs in %s hits", what); misses++; };
        miss(make_key(o, kind, 3, 1, 1, a), "N");
        miss(make_key(o, kind, 2, 2, 1, a), "win_B");
        miss(make_key(o, kind, 2, 1, 2, a), "win_S");
        const float *CallArgs::*ins[7] = {&CallArgs::tgt, &CallArgs::src, &CallArgs::depth_t, &CallArgs::depth_s, &CallArgs::K, &CallArgs::pose_in, &CallArgs::log_scale_in};
        float *CallArgs::*outs[4] = {&CallArgs::pose_out, &CallArgs::log_scale_out, &CallArgs::depth_out, &CallArgs::stats_out};
        int ptr_misses = 0;
        for (auto f : ins) {
            CallArgs b = a;
            b.*f = g_arrays + 12;
            if (kind == CALL_DENSE && f == &CallArgs::log_scale_in) { CHECK(c.sight(make_key(o, kind, 2, 1, 1, b), true, &ev) == SIGHT_REPLAY, "a dense call has no log-scale"); continue; }
            miss(make_key(o, kind, 2, 1, 1, b), "an input pointer"); ptr_misses++;
        }
        for (auto f : outs) {
            CallArgs b = a;
            b.*f = g_arrays + 13;
            const bool in_key = kind == CALL_DENSE ? f != &CallArgs::log_scale_out : f != &CallArgs::depth_out;
            if (!in_key) { CHECK(c.sight(make_key(o, kind, 2, 1, 1, b), true, &ev) == SIGHT_REPLAY, "a pointer the call does not take is in its key"); continue; }
            miss(make_key(o, kind, 2, 1, 1, b), "an output pointer"); ptr_misses++;
        }
        CHECK(ptr_misses == (kind == CALL_POSE ? 10 : 9), "pointers in the key: %d", ptr_misses);      // (slot 6 of a dense key is always null)
        for (size_t i = 0; i < sizeof(o); i++) {
            tcsfm_opts o2 = o;
            ((unsigned char *)&o2)[i] ^= 0x40;
            miss(make_key(o2, kind, 2, 1, 1, a), "a byte of the options");
        }
        CHECK(c.sight(k0, true, &ev) == SIGHT_REPLAY, "the base call is lost");
        (void)misses;
    }
    // ... and in `kind` ALONE: arguments whose ten pointer slots read the same as a pose call and as a dense call (no log_scale_in; the
    // pose call's log_scale_out is the dense call's depth_out), so that nothing but `kind` tells the two keys apart
    CallArgs same = a;
    same.log_scale_in = nullptr; same.log_scale_out = same.depth_out;
    const CallKey kp = make_key(o, CALL_POSE, 2, 1, 1, same), kd = make_key(o, CALL_DENSE, 2, 1, 1, same);
    CHECK(memcmp(kp.p, kd.p, sizeof(kp.p)) == 0 && memcmp(&kp.o, &kd.o, sizeof(kp.o)) == 0 && kp.N == kd.N && kp.win_B == kd.win_B && kp.win_S == kd.win_S,
          "the two keys differ in more than kind");
    // (kd is the dense base call above, captured as 101: a dense key does not read the log-scales)
    CHECK(c.sight(kd, true, &ev) == SIGHT_REPLAY && c.replay() == 100 + CALL_DENSE, "the dense call is not held");
    CHECK(c.sight(kp, true, &ev) == SIGHT_FIRST && ev == 0, "a key that differs in kind alone hits");
    CHECK(c.sight(kd, true, &ev) == SIGHT_REPLAY && c.replay() == 100 + CALL_DENSE, "the dense call no longer replays its own executable");
    CHECK(c.sight(kp, true, &ev) == SIGHT_CAPTURE, "the pose call of the same pointers is not an entry of its own");
    c.captured(200);
    CHECK(c.sight(kp, true, &ev) == SIGHT_REPLAY && c.replay() == 200 && c.sight(kd, true, &ev) == SIGHT_REPLAY && c.replay() == 100 + CALL_DENSE,
          "the two kinds share an executable");
    CHECK(c.drop_all().size() == 3, "drop_all");
    return scripts;
}

// ---- pose plan -------------------------------------------------------------------------------------------------------------------------
static void check_pose_plan() {
    for (int solver : {TCSFM_SOLVER_GN, TCSFM_SOLVER_LM})
        for (int n_iters = 0; n_iters <= 5; n_iters++) {
            const PosePlan p = pose_plan(3, 0, 0, 0, 0, 0, solver, n_iters, TCSFM_REFINE_POSE, 0);
            const bool lm = solver == TCSFM_SOLVER_LM;
            CHECK(p.n_lin == n_iters + (lm && n_iters ? 1 : 0) && p.n_lin == pose_n_lin(solver, n_iters), "n_lin %d", p.n_lin);
            CHECK(p.finish == (n_iters == 0), "k_finish at n_iters %d", n_iters);
            int emits = 0;
            for (int i = 0; i < p.n_lin; i++) {
                const PoseStep s = p.step(i);
                emits += s.emit ? 1 : 0;
                if (i < n_iters) CHECK(s.lin == POSE_STEP_LIN && s.it == i && s.solve_mode == 0 && s.emit == (!lm && i == n_iters - 1), "step %d of %d", i, n_iters);
                else CHECK(lm && i == n_iters && s.lin == POSE_STEP_COST && s.it == n_iters && s.solve_mode == 1 && s.emit, "the cost step");
            }
            CHECK(emits == (n_iters ? 1 : 0), "%d steps emit the pose", emits);      // (n_iters == 0: k_finish does)
        }
    // the hand-made table, at 17 x 33 = 561 pixels
    const size_t hw = 561;
    struct Row { int N, win_B, win_S, ncall, cB, cS, n_iters, refine, argmin; int np, nimg_t, nimg_s, rows, n_sel; size_t tgt, src, dt, ds, K, pose, ls, stats, maps; };
    const Row rows[] = {
        // the pair form: 3 pairs, an image set each
        {3, 0, 0, 0, 0, 0, 4, TCSFM_REFINE_POSE, 1, 6, 3, 3, 3, 0, 5049, 5049, 1683, 1683, 27, 18, 3, 150, 1683},
        // a 2 x 3 window: 12 directed pairs, 2 targets, 6 sources, a pack row per forward pair, the min over the sources on all 6
        {12, 2, 3, 0, 0, 0, 2, TCSFM_REFINE_POSE_SCALE, 1, 7, 2, 6, 6, 6, 3366, 10098, 1122, 3366, 18, 72, 12, 360, 6732},
        // ... without argmin, and with one source: no selection
        {12, 2, 3, 0, 0, 0, 2, TCSFM_REFINE_POSE, 0, 6, 2, 6, 6, 0, 3366, 10098, 1122, 3366, 18, 72, 12, 360, 6732},
        {4, 2, 1, 0, 0, 0, 0, TCSFM_REFINE_POSE, 1, 6, 2, 2, 2, 0, 3366, 3366, 1122, 1122, 18, 24, 4, 40, 2244},
        // three queued 1 x 2 calls merged: 12 pairs; the staged arrays are ONE call's (1 target, 2 sources)
        {12, 3, 2, 3, 1, 2, 4, TCSFM_REFINE_POSE, 1, 6, 1, 2, 6, 6, 1683, 3366, 561, 1122, 9, 72, 12, 600, 6732},
        // two queued 1 x 1 calls merged
        {4, 2, 1, 2, 1, 1, 4, TCSFM_REFINE_POSE_SCALE, 0, 7, 1, 1, 2, 0, 1683, 1683, 561, 561, 9, 24, 4, 200, 2244},
    };
    for (const Row &r : rows) {
        const PosePlan p = pose_plan(r.N, r.win_B, r.win_S, r.ncall, r.cB, r.cS, TCSFM_SOLVER_GN, r.n_iters, r.refine, r.argmin);
        CHECK(p.N == r.N && p.np == r.np && p.nimg_t == r.nimg_t && p.nimg_s == r.nimg_s && p.pack_rows == r.rows && p.n_sel == r.n_sel,
              "plan of N %d (%d x %d, %d calls): np %d sets %d / %d rows %d n_sel %d", r.N, r.win_B, r.win_S, r.ncall, p.np, p.nimg_t, p.nimg_s, p.pack_rows, p.n_sel);
        CHECK(p.tgt(hw) == r.tgt && p.src(hw) == r.src && p.depth_t(hw) == r.dt && p.depth_s(hw) == r.ds && p.K() == r.K && p.pose() == r.pose &&
              p.log_scale() == r.ls && p.stats() == r.stats && p.maps(hw) == r.maps, "extents of N %d (%d x %d, %d calls)", r.N, r.win_B, r.win_S, r.ncall);
        CHECK(p.window == (r.win_B > 0), "window form");
    }
}

int main() {
    const double q_scripts = check_queue();
    const long q_states = q_played;
    const long lane_cases = check_lanes();
    const double g_scripts = check_graphs();
    check_pose_plan();
    if (bad) { printf("call_plan_host: %d checks failed\n", bad); return 1; }
    printf("call_plan_host ok: %.0f queue scripts (played from %ld waiting states), %ld lane steps, %.0f graph scripts (played from %ld cache states), pose plan\n",
           q_scripts, q_states, lane_cases, g_scripts, g_played);
    return 0;
}
