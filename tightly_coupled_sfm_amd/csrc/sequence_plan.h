// The ring plan and the schedule of a sequence call (sequence_host.h), host only: which frames go up when, into which slots, behind which
// events, and which windows a call takes.  Integer arithmetic, no HIP, no environment: tests/asan/sequence_plan_host.cpp builds it alone
// and plays the schedule against a model of the slots.
//
// The pipeline.  Frames go up in CHUNKS of C on the copy stream into a ring of R slots (frame f lives in slot f % R); the first M slots
// are mirrored behind the ring (position R + s holds what slot s holds), so the WB + S frames of a CALL -- WB consecutive windows of
// S + 1 frames -- sit at consecutive positions and never wrap.  A chunk's stages (bytes to floats, depth, scale, pack) run on the pack
// stream behind its copy; the chunk's event (seq_copied) is recorded after the last of them.  Calls go round the L lanes (call ci on
// lane ci % L); a call waits for the chunk events of its frames and records its done-event (seq_done) when it has been issued.
//
// Why nothing races: the invariants.  tests/asan/sequence_plan_host.cpp checks each of them over a grid of parameters.
//  1. at() is a bijection onto [0, nwin * N): every pair of every window has its own place in the per-call pose staging.
//  2. Frames go up once each, in order, all T of them by the last call, and a chunk never crosses the end of the ring (slot + nf <= R).
//  3. A chunk goes up only when every window that reads a frame it overwrites has been ISSUED (nxt + C - 1 - R < c0): the readers'
//     done-events exist, so the copy can wait for them.
//  4. The copy waits for the latest reader of its slots and the L - 1 calls before it: one per lane, and a lane's stream is in order, so
//     for every reader.  Those calls still own their events: seq_done[r % ND] was last recorded by r (ND = 2 R + 1 events for calls,
//     far more than the calls whose slots can be pending).
//  5. When a call is issued, every chunk event it waits for was last recorded by the chunk that holds the call's frames, not by a later
//     chunk in the same slots (a later one needs the call issued first: 3).
//  6. The call's nbw + S frames sit at positions s0 .. s0 + nbw + S - 1 < R + M, mirror slots included, and position s0 + k holds
//     exactly frame c0 + k.
//  7. The done-event the host throttles on was recorded by a call in [ci - depth, ci): the host is never more than `depth` calls ahead.
//     (With a small explicit ring ND can be smaller than depth -- ring = 3, S = 1: ND = 7, depth = 16 -- and the event at
//     (ci - depth) % ND has been re-recorded by a later call, ci - 2 in the example.  The host then waits for MORE than it has to,
//     which is harmless, and is kept.)
// What a stage may do follows from these.  A stage that runs on the pack stream between the chunk's copy (seq_raw) and its seq_copied
// record may read and write the chunk's own slots (and their mirrors): its writes come after the previous frames' readers (the copy
// waited for them: 4, and the stage waits for the copy), and the next copy into these slots waits for this chunk's readers (4), which
// waited for seq_copied (5), hence for the stage.  Anything indexed by the ABSOLUTE frame is never recycled and needs no argument.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace tc {

struct SeqPlan {
    static constexpr int kMaxOff = 8;      // sources per window at most (kernels.h: TC_MAX_SRC_OFF)
    int T = 0, S = 0, L = 0;               // frames, sources per window, lanes
    int N = 0, nwin = 0;                   // pairs per window (2 S), windows (T - S)
    int WB = 0, C = 0, R = 0, M = 0;       // windows per call, frames per chunk, ring slots, mirror slots
    int tp = 0, off[kMaxOff] = {};         // position of the target among a window's S + 1 frames; source s = frame w + off[s]
    int ahead = 0, ND = 0;                 // frames kept in flight ahead of a call's first window; done-events of calls
    long long depth = 0;                   // calls the host may run ahead of the GPU

    int nbw(int c0) const { return std::min(WB, nwin - c0); }      // windows of the call that starts at window c0
    // Poses live on the device per CALL in the stacked order of the window form (forward pairs (s, b), then inverse pairs); the
    // caller's arrays are per window.  at(): offset (in pairs) of pair j of window w inside the staging arrays.
    size_t at(int w, int j) const {
        const int c0 = (w / WB) * WB, n = nbw(c0), b = w - c0;
        return (size_t)c0 * N + (j < S ? (size_t)j * n + b : (size_t)S * n + (size_t)(j - S) * n + b);
    }
};

// The plan of a call on T frames with S sources per window over L lanes; max_images: the PoseNet's (0: none); chunk_override: the
// TCSFM_SEQ_CHUNK measurement hook (0: none).  The caller has checked S >= 1, T > S, 2 S <= max_pairs (<= max_images),
// windows_per_call >= 0 and -1 <= target_pos <= S <= kMaxOff.  Returns NULL, or why the ring is refused (the plan is filled in either way).
inline const char *seq_plan(int T, int S, int L, int max_pairs, int max_images, int ring, int windows_per_call, int target_pos,
                            int chunk_override, SeqPlan &p) {
    p.T = T; p.S = S; p.L = L; p.N = 2 * S; p.nwin = T - S;
    // position of the target inside a window's S + 1 consecutive frames: the reference's loaders take the middle one
    // (data/kitti_loader.py:271-273: target_idx = int(len / 2), the sources are the others in order)
    p.tp = target_pos < 0 ? (S + 1) / 2 : target_pos;
    for (int s = 0; s < SeqPlan::kMaxOff; s++) p.off[s] = s < p.tp ? s : s + 1;
    // Windows per call: consecutive windows are independent, and the targets (frames w + tp ..) and every source (frames w + off[s] ..)
    // of WB consecutive windows are runs of the ring -- the window form with explicit source positions -- so a lane refines WB windows
    // per call: the kernels fill the chip (26 200 windows/s per call at WB = 8 against 13 900 at WB = 1) and the PoseNet runs on
    // 2 S WB images at a third of the time per image.
    int WB = windows_per_call > 0 ? windows_per_call : 8;
    WB = std::min(WB, std::min(max_pairs / p.N, p.nwin));
    if (max_images > 0) WB = std::min(WB, max_images / p.N);
    while (ring > 0 && WB > 1 && ring < WB + S + (ring >= WB + S + 8 ? 4 : 1)) WB--;      // an explicit small ring bounds the windows per call
    p.WB = WB;
    // frames go up in chunks of C (one copy for the images, one for the depths: PCIe runs at 55 GB/s on 8-frame copies, at 36 GB/s on
    // single frames, and the host issues a quarter of the calls); the ring holds a whole number of chunks.  Default ring: 4 frames per
    // copy; 8 when a call takes 16 or more windows (the copies then run at 55 instead of 45 GB/s and a call still waits for no more
    // than two of them: 21 800 -> 22 800 windows/s at 16 windows per call, nothing to gain at 8)
    p.C = ring > 0 ? (ring >= WB + S + 8 ? 4 : 1) : (chunk_override ? chunk_override : (WB >= 16 ? 8 : 4));
    p.R = ring > 0 ? (ring / p.C) * p.C : ((32 + (L + 1) * WB + S + p.C - 1) / p.C) * p.C;     // frames resident at once
    p.M = WB + S - 1;                      // mirror slots behind the ring: the WB + S frames of a call never wrap
    p.ahead = S + L * WB + p.C;
    p.depth = std::max(2 * L, 16 / WB);
    p.ND = 2 * p.R + 1;                    // a call's event is re-recorded long after its slots were recycled
    if (p.R < S + 2 || p.R < WB + S + p.C)
        return "tcsfm_refine_sequence: ring must hold at least windows_per_call + S + 4 frames (S + 2 for one window per call)";
    return nullptr;
}

// One chunk of frames on its way up: frames first .. first + nf - 1 into slots slot .., the first nm of them mirrored at R + slot ..
struct SeqChunk {
    int first, nf, slot, nm;
    int ev;                                // index of its seq_raw / seq_copied event
    long long wait_last; int n_wait;       // the copy waits for the done-events of calls wait_last, wait_last - 1, .. (n_wait of them)
};

// The schedule of an accepted plan.  Per call (ci, c0, nbw), in this order: throttle_event, next_chunk until it says no, lane_waits,
// and issued once the call's done-event has been recorded.  Events are handed out as indices: done_event into seq_done (ND of them),
// the chunks' into seq_raw / seq_copied (R / C at most R of them).
class SeqSchedule {
  public:
    explicit SeqSchedule(const SeqPlan &plan) : p(plan), slot_reader((size_t)plan.R, -1) {}
    int done_event(long long call) const { return (int)(call % p.ND); }
    // the done-event the host waits for before it issues call ci (-1: none): the host stays a bounded number of calls ahead of the GPU.
    // A deeper backlog buys nothing, and with one the runtime was seen to block a single hipMemcpyAsync of the copy stream for 7 ms
    // while the lanes ran dry behind it.  (Invariant 7: with ND < depth the event belongs to a later call and the host waits for more.)
    int throttle_event(long long ci) const { return ci >= p.depth ? done_event(ci - p.depth) : -1; }
    // the next chunk that goes up before the call at window c0, if any: frames are kept `ahead` in flight, and a chunk may go up once
    // every window that reads the frames it overwrites has been issued (invariant 3)
    bool next_chunk(int c0, int nbw, SeqChunk &c) {
        if (!(nxt < p.T && nxt <= c0 + nbw - 1 + p.ahead && nxt + p.C - 1 - p.R < c0)) return false;
        c.first = nxt; c.slot = nxt % p.R; c.nf = p.T - nxt < p.C ? p.T - nxt : p.C;
        c.nm = c.slot < p.M ? (c.nf < p.M - c.slot ? c.nf : p.M - c.slot) : 0;
        c.ev = c.slot / p.C;
        long long last = -1;               // the slots' previous frames may still be read: the copy waits for their readers --
        for (int k = 0; k < c.nf; k++) { if (slot_reader[c.slot + k] > last) last = slot_reader[c.slot + k]; slot_reader[c.slot + k] = -1; }
        c.wait_last = last; c.n_wait = 0;  // -- the latest of those calls on every lane (a lane's stream is in order)
        for (long long r = last; r >= 0 && r > last - p.L; r--) c.n_wait++;
        nxt += c.nf;
        return true;
    }
    // the chunk events the lane waits for before the call: those of the chunks that hold frames c0 .. c0 + nbw - 1 + S
    void lane_waits(int c0, int nbw, std::vector<int> &ev) const {
        ev.clear();
        for (int k = c0 / p.C; k <= (c0 + nbw - 1 + p.S) / p.C; k++) ev.push_back((k * p.C % p.R) / p.C);
    }
    // call ci has been issued: it is the reader of its frames' slots
    void issued(long long ci, int c0, int nbw) {
        for (int k = 0; k < nbw + p.S; k++) slot_reader[(c0 + k) % p.R] = ci;
    }

  private:
    const SeqPlan &p;
    std::vector<long long> slot_reader;    // last CALL that reads the frame in this slot (-1: none pending)
    int nxt = 0;                           // first frame of the next chunk
};

}  // namespace tc
