// Stand-alone sanitizer program for the ring plan and the schedule of the sequence calls (csrc/sequence_plan.h).  Its own main, no
// Python, no GPU:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I tightly_coupled_sfm_amd/csrc tests/asan/sequence_plan_host.cpp -o sequence_plan_host && ./sequence_plan_host
//
// (the runtimes are linked statically: the program then runs as it is wherever the process's library list does not start with them)
// Every accepted plan of a grid of parameters is played, call by call, against a model of the slots (ring + mirror) and of the events,
// and the seven invariants at the top of sequence_plan.h are checked as the schedule goes; a table pins the plans of the parameters
// the GPU tests and the timing scripts use, so that a plan that quietly picks fewer windows per call (same results, half the speed)
// fails here.
#include <stdio.h>
#include <vector>
#include "sequence_plan.h"

using tc::SeqChunk;
using tc::SeqPlan;
using tc::SeqSchedule;

// plays the schedule of an accepted plan; 0, or the number of the invariant that broke (x 10 + a sub-check)
static int play(const SeqPlan &p) {
    {   // 1: at() is a bijection onto [0, nwin * N)
        std::vector<char> seen((size_t)p.nwin * p.N, 0);
        for (int w = 0; w < p.nwin; w++)
            for (int j = 0; j < p.N; j++) {
                const size_t a = p.at(w, j);
                if (a >= seen.size() || seen[a]) return 10;
                seen[a] = 1;
            }
    }
    if (p.R % p.C != 0) return 20;
    SeqSchedule sched(p);
    std::vector<int> frame_at((size_t)p.R + p.M, -1);              // the frame each position (ring, then mirror) holds
    std::vector<long long> reader((size_t)p.R, -1);                // the model's own: latest call that read the frame in this slot
    std::vector<long long> done_rec((size_t)p.ND, -1);             // last call that recorded this done-event
    std::vector<int> chunk_rec((size_t)p.R / p.C, -1);             // first frame of the last chunk that recorded this chunk event
    std::vector<int> waits;
    int uploaded = 0, issued_upto = 0;                             // frames gone up; windows issued
    long long ci = 0;
    for (int c0 = 0; c0 < p.nwin; c0 += p.WB, ci++) {
        const int nbw = p.nbw(c0);
        const int te = sched.throttle_event(ci);
        if (te >= 0) {     // 7 (as worded there: at least as late as ci - depth, and an earlier call than this one)
            if (te >= p.ND) return 70;
            if (done_rec[te] < ci - p.depth || done_rec[te] >= ci) return 71;
        } else if (ci >= p.depth) return 72;
        SeqChunk c;
        while (sched.next_chunk(c0, nbw, c)) {
            if (c.first != uploaded || c.nf < 1 || c.nf > p.C) return 21;                       // 2: once each, in order
            if (c.slot != c.first % p.R || c.slot + c.nf > p.R) return 22;                      // 2: never across the end of the ring
            if (c.nm != std::max(0, std::min(c.nf, p.M - c.slot))) return 23;
            if (c.ev < 0 || c.ev >= (int)chunk_rec.size() || c.ev != c.slot / p.C) return 24;
            for (long long i = 0; i < c.n_wait; i++) {                                          // 4: the waited calls own their events
                const long long r = c.wait_last - i;
                if (r < 0 || r >= ci || done_rec[sched.done_event(r)] != r) return 40;
            }
            for (int k = 0; k < c.nf; k++) {
                const int old = frame_at[c.slot + k];
                if (old >= 0 && std::min(old, p.nwin - 1) >= issued_upto) return 30;            // 3: its last reader (window min(old, nwin - 1)) is issued
                if (c.slot + k < p.M && frame_at[p.R + c.slot + k] != old) return 31;           // (the mirror held the same frame)
                const long long r = reader[c.slot + k];                                         // 4: every reader is covered, lane by lane
                if (r >= 0) {
                    bool covered = false;
                    for (long long i = 0; i < c.n_wait; i++)
                        if ((c.wait_last - i) % p.L == r % p.L && c.wait_last - i >= r) covered = true;
                    if (!covered) return 41;
                }
                reader[c.slot + k] = -1;
                frame_at[c.slot + k] = c.first + k;
                if (k < c.nm) frame_at[p.R + c.slot + k] = c.first + k;
            }
            chunk_rec[c.ev] = c.first;
            uploaded += c.nf;
        }
        sched.lane_waits(c0, nbw, waits);      // 5: the events of the chunks that hold frames c0 .. c0 + nbw - 1 + S, each last recorded by that chunk
        const int k0 = c0 / p.C, k1 = (c0 + nbw - 1 + p.S) / p.C;
        if ((int)waits.size() != k1 - k0 + 1) return 50;
        for (int k = k0; k <= k1; k++) {
            const int e = waits[k - k0];
            if (e < 0 || e >= (int)chunk_rec.size() || chunk_rec[e] != k * p.C) return 51;
        }
        const int s0 = c0 % p.R;               // 6: consecutive positions, each holding its frame
        if (s0 + nbw + p.S - 1 >= p.R + p.M) return 60;
        for (int k = 0; k < nbw + p.S; k++) {
            if (frame_at[s0 + k] != c0 + k) return 61;
            reader[(s0 + k) % p.R] = ci;       // (position R + s is slot s)
        }
        done_rec[sched.done_event(ci)] = ci;
        sched.issued(ci, c0, nbw);
        issued_upto = c0 + nbw;
    }
    if (uploaded != p.T || issued_upto != p.nwin) return 25;       // 2: all T frames by the last call
    return 0;
}

struct Row { int T, S, L, max_pairs, ring, wpc, max_images, chunk; int WB, C, R, M; };      // WB = 0: refused

int main() {
    int bad = 0;
    // the plans of the parameters tests/test_gpu_sequence.py and the timing scripts use
    const Row rows[] = {
        {30, 1, 1, 64, 0, 0, 0, 0, 8, 4, 52, 8},     {30, 1, 3, 64, 0, 0, 0, 0, 8, 4, 68, 8},      {30, 1, 2, 64, 4, 0, 0, 0, 2, 1, 4, 2},
        {30, 1, 3, 64, 12, 0, 0, 0, 8, 1, 12, 8},    {30, 2, 3, 64, 0, 0, 0, 0, 8, 4, 68, 9},      {30, 2, 2, 64, 5, 0, 0, 0, 2, 1, 5, 3},
        {30, 2, 2, 64, 12, 0, 0, 0, 8, 1, 12, 9},    {40, 2, 2, 64, 0, 3, 0, 0, 3, 4, 44, 4},      {40, 2, 1, 64, 12, 5, 0, 0, 5, 1, 12, 6},
        {40, 2, 3, 64, 20, 4, 0, 0, 4, 4, 20, 5},    {40, 2, 2, 64, 16, 8, 0, 0, 8, 1, 16, 9},     {40, 2, 2, 64, 6, 8, 0, 0, 3, 1, 6, 4},
        {200, 1, 2, 64, 0, 16, 0, 0, 16, 8, 88, 16}, {200, 2, 2, 64, 0, 16, 0, 0, 16, 8, 88, 17},  {200, 2, 2, 16, 0, 8, 0, 0, 4, 4, 48, 5},
        {9, 4, 2, 64, 0, 0, 0, 0, 5, 4, 52, 8},      {40, 1, 1, 16, 3, 0, 0, 0, 1, 1, 3, 1},       {40, 2, 1, 64, 3, 0, 0, 0, 0, 0, 0, 0},
        {40, 2, 2, 64, 3, 1, 0, 0, 0, 0, 0, 0},
        {30, 2, 2, 64, 0, 0, 8, 0, 2, 4, 40, 3},     // a PoseNet of 8 images holds 2 windows of 4 pairs: R = 32 + 3 * 2 + 2 rounded up to 4s
        {30, 1, 2, 64, 0, 0, 0, 2, 8, 2, 58, 8},     // the chunk override: C = 2, R = 32 + 3 * 8 + 1 rounded up to 2s
        {30, 1, 2, 64, 12, 0, 0, 2, 8, 1, 12, 8},    // ... which an explicit ring ignores
    };
    for (const Row &r : rows) {
        SeqPlan p;
        const char *why = tc::seq_plan(r.T, r.S, r.L, r.max_pairs, r.max_images, r.ring, r.wpc, -1, r.chunk, p);
        const bool same = r.WB == 0 ? why != nullptr : (!why && p.WB == r.WB && p.C == r.C && p.R == r.R && p.M == r.M);
        if (!same) {
            printf("plan T %d S %d L %d max_pairs %d ring %d wpc %d max_images %d chunk %d: %s WB %d C %d R %d M %d, expected WB %d C %d R %d M %d\n", r.T, r.S,
                   r.L, r.max_pairs, r.ring, r.wpc, r.max_images, r.chunk, why ? "refused;" : "", p.WB, p.C, p.R, p.M, r.WB, r.C, r.R, r.M);
            bad++;
        } else if (!why) {
            if (int rc = play(p)) { printf("table plan T %d S %d L %d ring %d wpc %d: check %d failed\n", r.T, r.S, r.L, r.ring, r.wpc, rc); bad++; }
        }
    }
    // the grid; every target position for the small T, the default one otherwise
    const int Ts[] = {2, 3, 5, 9, 17, 40, 101}, Ss[] = {1, 2, 3, 4, 8}, Ls[] = {1, 2, 3, 4}, rings[] = {0, 3, 4, 5, 6, 12, 16, 20, 33};
    const int wpcs[] = {0, 1, 2, 3, 5, 8, 16}, mps[] = {16, 64};
    int accepted = 0, refused = 0;
    for (int T : Ts) for (int S : Ss) for (int L : Ls) for (int ring : rings) for (int wpc : wpcs) for (int mp : mps) {
        if (T <= S || 2 * S > mp) { refused++; continue; }         // (the driver's own first check)
        SeqPlan p;
        if (tc::seq_plan(T, S, L, mp, 0, ring, wpc, -1, 0, p)) { refused++; continue; }
        accepted++;
        if (p.N != 2 * S || p.nwin != T - S || p.tp != (S + 1) / 2 || p.M != p.WB + S - 1 || p.ND != 2 * p.R + 1) { printf("plan fields\n"); bad++; }
        if (int rc = play(p)) { printf("T %d S %d L %d ring %d wpc %d max_pairs %d: check %d failed\n", T, S, L, ring, wpc, mp, rc); bad++; }
    }
    if (accepted != 10976 || refused != 6664) { printf("grid: %d accepted, %d refused; 10976 and 6664 expected\n", accepted, refused); bad++; }
    for (int tpos = 0; tpos <= 3; tpos++) {                        // the source offsets skip the target's position
        SeqPlan p;
        tc::seq_plan(17, 3, 2, 64, 0, 0, 0, tpos, 0, p);
        for (int s = 0; s < 3; s++)
            if (p.tp != tpos || p.off[s] != (s < tpos ? s : s + 1)) { printf("off[] at target_pos %d\n", tpos); bad++; }
    }
    printf(bad ? "FAILED\n" : "sequence_plan_host ok: %d plans played, %d refused\n", accepted, refused);
    return bad ? 1 : 0;
}
