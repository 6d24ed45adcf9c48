// Host side of the sequence calls: the reference's sequential driver (run_sequential_optimization.py:186-247) as ONE call, see
// include/tcsfm.h -- the three entry points, the settings of their stages and what they keep.  The ring arithmetic and the schedule are
// sequence_plan.h's (no HIP there), with the argument why nothing races at its top; here is what goes on which stream.  Part of
// tcsfm_api.hip, the library's only translation unit: included after posenet_host.h and depthnet_host.h (pose_loop, pn_for_lane,
// dn_sequence_depths, dn_post_scratch) and the helpers launch_frame_scales, launch_resize_u8, launch_frames_u8, resize_table and
// flip_ramp_device.
#pragma once
#include "sequence_plan.h"

namespace {

static_assert(SeqPlan::kMaxOff == TC_MAX_SRC_OFF, "the plan's source offsets are WinOff's");

// One sequence call: its arguments, the plan, what is switched on, the lanes -- and the steps, in the order run() takes them.  A step
// returns a refusal or a failed HIP call, which ends the call at once; a failed launch sequence (dn_sequence_depths, pose_loop,
// refine_impl, dense_impl) goes into `failed`: the loop ends and the drain returns it.
struct SeqCall {
    tcsfm_ctx *h;
    const char *entry;
    int T, S;
    const float *frames, *depths, *K, *pose_init;
    tcsfm_posenet *pn;             // with it the initial poses of every window come from the coupled PoseNet loop (train_mono.py:64-80) on the
    int num_iter;                  // window's lane instead of from the caller
    float *pose_init_out, *pose_out, *log_scale_out, *dense_depth_out;
    tcsfm_opts o;
    SeqPlan p;
    WinOff wo;
    bool gen;                      // depths == NULL: the attached depth network (tcsfm_sequence_depthnet) computes every frame's depth as its chunk lands
    bool u8;                       // tcsfm_sequence_frame_format: `frames` points at bytes; they go up as they are and k_frames_u8 makes the ring's floats
    bool resize;                   // tcsfm_sequence_frame_source: the bytes are camera-size frames; k_resize_u8 takes k_frames_u8's place
    bool scale_on;                 // tcsfm_sequence_scale: every frame's DNet scale from the ring's depth plane, on the pack stream
    bool dense, use_cache;         // tcsfm_refine_dense_sequence; the frame-level pack cache (the dense modes rewrite per-pair depth planes: they keep the per-pair pack)
    bool staged;                   // the chunk has a stage on seq_pack: k_frames_u8, the depth network, the scale stage and / or k_frame_pack
    int disp_mode;                 // tcsfm_sequence_disparity: every frame's disparity kept on the device
    size_t frame_bytes, hw;        // bytes of one frame of a U8 format; H W
    int np;
    const ResizeTable *rtab = nullptr;
    const double *disp_ramp = nullptr;
    float gen_min_disp = 0.f, gen_max_disp = 0.f;      // tcsfm_disp_to_depth's arguments
    std::vector<tcsfm_ctx *> lane;
    std::vector<tcsfm_posenet *> net;
    std::vector<hipStream_t> ls;
    std::vector<float> stage;      // host staging of the per-window arrays
    std::vector<int> waits;
    int failed = TCSFM_OK;

    // somebody reads the RAW mirror slots of a chunk with nm mirrored frames: with the pack cache only the PoseNet does
    bool raw_mirror(int nm) const { return nm > 0 && (!use_cache || pn); }
    float *img(int pos) const { return h->seq_img.p + (size_t)pos * 3 * hw; }
    float *depth(int pos) const { return h->seq_depth.p + (size_t)pos * hw; }

    int check(const tcsfm_opts *o_in, int ring, int windows_per_call, int target_pos);
    int reserve();
    int upload_small();
    int stage_chunk(const SeqSchedule &sched, const SeqChunk &ch);
    int issue_call(const SeqSchedule &sched, long long ci, int c0, int nbw);
    int drain_fetch();
    int run(const tcsfm_opts *o_in, int ring, int windows_per_call, int target_pos);
};

// Step 1: everything that can refuse the call, in a fixed order (the refusal tests assert which message a bad input gets); fills in the
// flags and the plan.  What sequence_plan.h has against the ring is reported last, where it always was.  Nothing here touches the device.
int SeqCall::check(const tcsfm_opts *o_in, int ring, int windows_per_call, int target_pos) {
    const int N = 2 * S, L = h->lanes_serial ? 1 : (int)h->lanes.size() + 1;
    if (S < 1 || T <= S || N > h->max_pairs) return fail(h, TCSFM_E_ARG, "tcsfm_refine_sequence: need S >= 1, T > S and 2*S <= max_pairs");
    gen = !depths && h->seq_dn;
    u8 = h->seq_fmt != TCSFM_FRAMES_F32_CHW;
    resize = h->seq_src_h > 0;
    if (resize && !u8)
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": a frame source size (tcsfm_sequence_frame_source) needs a U8 frame format, not TCSFM_FRAMES_F32_CHW").c_str());
    frame_bytes = resize ? (size_t)3 * h->seq_src_h * h->seq_src_w : (size_t)3 * h->H * h->W;
    hw = (size_t)h->H * h->W;
    disp_mode = h->seq_disp_mode;         // the stage needs the attached network's own output
    if (disp_mode != TCSFM_SEQ_DISP_OFF && depths)
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": the disparity stage (tcsfm_sequence_disparity) needs depths == NULL: it keeps the attached depth network's own output").c_str());
    if (disp_mode != TCSFM_SEQ_DISP_OFF && !h->seq_dn)
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": the disparity stage (tcsfm_sequence_disparity) needs an attached depth network (tcsfm_sequence_depthnet)").c_str());
    if (!frames || (!depths && !gen) || !K || (!pose_init && !pn) || !pose_out) return fail(h, TCSFM_E_ARG, "tcsfm_refine_sequence: NULL input");
    if (gen && o_in->depth_is_disp)
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": depths == NULL (the attached depth network produces depths) cannot go with opts.depth_is_disp").c_str());
    if (gen && !(o_in->min_depth > 0 && o_in->max_depth > o_in->min_depth)) return fail(h, TCSFM_E_ARG, "min_depth/max_depth invalid");
    scale_on = h->seq_cam_height > 0.f;
    if (scale_on && o_in->depth_is_disp)
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": the scale stage (tcsfm_sequence_scale) needs depths, not disparities (opts.depth_is_disp)").c_str());
    if (scale_on && (h->H < 5 || h->W < 5))
        return fail(h, TCSFM_E_ARG, (std::string(entry) + ": the scale stage (tcsfm_sequence_scale): image too small").c_str());
    if (windows_per_call < 0) return fail(h, TCSFM_E_ARG, "tcsfm_refine_sequence: windows_per_call < 0");
    if (target_pos < -1 || target_pos > S || S > TC_MAX_SRC_OFF) return fail(h, TCSFM_E_ARG, "tcsfm_refine_sequence: target_pos must be -1 or 0..S, S at most 8");
    {   // The overlap contract (include/tcsfm.h).  Host arrays that are streamed: frames and depths are still going up while results come
        // back, so only the pose pair is honoured -- pose_init is on the device, and the copy stream drained, before the first window is
        // issued (upload_small), and pose_out is written after the last one has finished.
        const size_t hw_b = hw * sizeof(float), np6 = (size_t)(T - S) * N * 6 * sizeof(float);
        ArgRanges a;
        a.in("frames", frames, u8 ? (size_t)T * frame_bytes : (size_t)T * 3 * hw_b);      // (a U8 format: T*3*H*W -- T*3*src_h*src_w -- bytes, not floats)
        a.in("depths", depths, (size_t)T * hw_b); a.in("K", K, 9 * sizeof(float));
        a.in("pose_init", pose_init, np6);
        a.out("pose_init_out", pose_init_out, np6); a.out("pose_out", pose_out, np6);
        if (o_in->refine == TCSFM_REFINE_POSE_SCALE && !dense_depth_out) a.out("log_scale_out", log_scale_out, (size_t)(T - S) * N * sizeof(float));
        a.out("depth_out", dense_depth_out, (size_t)(T - S) * N * hw_b);
        a.bless("pose_out", "pose_init");
        std::string msg;
        if (a.refused(entry, msg)) return fail(h, TCSFM_E_ARG, msg.c_str());
    }
    if (pn && (num_iter < 1 || pn->h != h || !pn->loaded || N > pn->max_images || o_in->depth_is_disp))
        return fail(h, TCSFM_E_ARG, "tcsfm_odometry_sequence: needs a loaded PoseNet of this handle with max_images >= 2*S, num_iter >= 1 and depths (not disparities)");
    o = *o_in;
    o.host_ptrs = 0;                                   // the lanes work on the device ring; this call does the staging itself
    static const int chunk_env = getenv("TCSFM_SEQ_CHUNK") ? std::max(1, atoi(getenv("TCSFM_SEQ_CHUNK"))) : 0;      // (measurement hook)
    const char *ring_refusal = seq_plan(T, S, L, h->max_pairs, pn ? pn->max_images : 0, ring, windows_per_call, target_pos, chunk_env, p);
    wo.on = 1;
    for (int s = 0; s < TC_MAX_SRC_OFF; s++) wo.off[s] = p.off[s];      // source s = frame w + off[s], relative to the window's first frame
    if (int rc = check_common(h, &o, N * p.WB)) return rc;
    if (K[1] != 0.f || K[3] != 0.f || K[6] != 0.f || K[7] != 0.f || K[8] != 1.f || !(K[0] != 0.f) || !(K[4] != 0.f))
        return fail(h, TCSFM_E_INTRINSICS, "intrinsics must be pinhole [fx 0 cx; 0 fy cy; 0 0 1]");
    if (int rc = pending_error(h)) return rc;
    if (ring_refusal) return fail(h, TCSFM_E_ARG, ring_refusal);
    dense = dense_depth_out != nullptr;
    use_cache = !dense;
    staged = use_cache || gen || u8 || scale_on;
    np = np_of(&o);
    if (gen) { gen_min_disp = 1.f / o.max_depth; gen_max_disp = 1.f / o.min_depth; }
    return TCSFM_OK;
}

// Step 2: scratch (ring + mirror slots, pose staging, WB copies of K, what the stages keep), streams, events and the lanes
int SeqCall::reserve() {
    const size_t slots = (size_t)p.R + p.M, pairs = (size_t)p.nwin * p.N;
    RESERVE(h, h->seq_img, slots * 3 * hw);
    RESERVE(h, h->seq_depth, slots * hw);
    if (u8) RESERVE(h, h->seq_u8, (size_t)p.R * frame_bytes);      // the byte ring: R slots, no mirror (the kernel writes the float mirror slots itself)
    if (resize && !(rtab = resize_table(h, h->seq_src_h, h->seq_src_w))) return TCSFM_E_HIP;
    if (use_cache) {           // the cache follows the ring's slot count (the largest so far)
        RESERVE(h, h->seq_fpack, h->seq_depth.cap / hw * (h->H + 2) * (h->W + 2));
        RESERVE(h, h->seq_fdepth, h->seq_depth.cap);
    }
    RESERVE(h, h->seq_pose_in, pairs * 6);
    RESERVE(h, h->seq_pose_out, pairs * 6);
    RESERVE(h, h->seq_ls_out, pairs);
    if (dense) RESERVE(h, h->seq_dense, pairs * hw);
    RESERVE(h, h->seq_K, (size_t)p.WB * 9);
    if (scale_on) {            // key planes of one chunk; results of every frame of the sequence
        RESERVE(h, h->seq_scale_keys, (size_t)p.C * hw);
        RESERVE(h, h->seq_scale_dev, (size_t)3 * T);
    }
    if (disp_mode != TCSFM_SEQ_DISP_OFF) {                 // every frame's plane, by absolute frame index; grown when a call needs more
        RESERVE(h, h->seq_disp_dev, (size_t)T * hw * (disp_mode == TCSFM_SEQ_DISP_POST ? sizeof(double) : sizeof(float)));
        if (disp_mode == TCSFM_SEQ_DISP_POST) {            // the clone's two planes of one group and the ramp
            if (int rc = dn_post_scratch(h->seq_dn->seq_clone.get(), entry)) return rc;
            if (!(disp_ramp = flip_ramp_device(h))) return TCSFM_E_HIP;
        }
    }
    if (!h->seq_copy) {   // high priority: a hardware queue outside the pool the normal-priority streams share (a copy stream that lands in
        int lo = 0, hi = 0;   // a lane's queue parks its slot-recycling waits in front of that lane's kernels), and copies go first anyway
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(h, h->seq_copy.create_with_priority(hi));
    }
    HIPCHK(h, h->seq_copied.grow((size_t)p.R));
    HIPCHK(h, h->seq_raw.grow(staged ? (size_t)p.R : 0));
    if (staged && !h->seq_pack) HIPCHK(h, h->seq_pack.create());
    HIPCHK(h, h->seq_done.grow((size_t)p.ND + 1));      // the calls' ND and one for the small inputs
    lane.resize(p.L); net.assign(p.L, nullptr); ls.resize(p.L);
    for (int l = 0; l < p.L; l++) {
        tcsfm_ctx *c = lane[l] = l == 0 ? h : h->lanes[l - 1];
        if (pn && !(net[l] = pn_for_lane(pn, c))) return fail(h, TCSFM_E_NOMEM, "tcsfm_odometry_sequence: no memory for a lane's PoseNet activations");
        ls[l] = l == 0 ? h->stream : c->own_stream;
        c->stream = ls[l];
        k_add(c, h->seq_K.p, p.WB);          // validated on the host (check)
        if (dense) RESERVE(h, c->seq_dense_tmp, (size_t)p.WB * p.N * hw);      // the lane's stacked maps of one call
    }
    return TCSFM_OK;
}

// Step 3: the small inputs, one copy each on the copy stream, and the host waits for them: every lane's first call comes later
int SeqCall::upload_small() {
    hipStream_t cs = h->seq_copy;
    std::vector<float> Kh((size_t)p.WB * 9);
    for (int b = 0; b < p.WB; b++) memcpy(&Kh[(size_t)b * 9], K, 9 * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(h->seq_K.p, Kh.data(), Kh.size() * sizeof(float), hipMemcpyHostToDevice, cs));
    if (!pn) {
        const float *src = pose_init;
        if (p.WB > 1) {        // the caller's arrays are per window, the device's per call (SeqPlan::at)
            stage.resize((size_t)p.nwin * p.N * 6);
            for (int w = 0; w < p.nwin; w++)
                for (int j = 0; j < p.N; j++) memcpy(&stage[p.at(w, j) * 6], pose_init + ((size_t)w * p.N + j) * 6, 6 * sizeof(float));
            src = stage.data();
        }
        HIPCHK(h, hipMemcpyAsync(h->seq_pose_in.p, src, (size_t)p.nwin * p.N * 6 * sizeof(float), hipMemcpyHostToDevice, cs));
    }
    hipEvent_t small_ev = h->seq_done[p.ND];
    HIPCHK(h, hipEventRecord(small_ev, cs));
    HIPCHK(h, hipEventSynchronize(small_ev));              // Kh / stage are host temporaries (pageable): gone from here on
    if (gen) {             // the network's weights may still be being written on the handle's stream (tcsfm_depthnet_load_device is asynchronous)
        HIPCHK(h, hipEventRecord(small_ev, h->stream));    // (small_ev is free again: the host has just waited for it)
        HIPCHK(h, hipStreamWaitEvent(h->seq_pack, small_ev, 0));
    }
    return TCSFM_OK;
}

// Step 4: one chunk goes up and through its stages.  The copy runs on the copy stream behind the done-events of the calls that read
// the slots' previous frames; the stages run on the PACK stream behind the raw frames (seq_raw), so that the next chunk's copy does not
// queue behind their kernels (a sequence with S = 1 is PCIe-bound: the copy stream is its critical path); seq_copied is recorded last.
// Every stage reads and writes this chunk's slots (and mirrors) or arrays indexed by the absolute frame: sequence_plan.h says why that
// is enough.
int SeqCall::stage_chunk(const SeqSchedule &sched, const SeqChunk &ch) {
    const int slot = ch.slot, nf = ch.nf, nm = ch.nm, mslot = p.R + slot;
    hipStream_t cs = h->seq_copy, ps = h->seq_pack;
    for (int i = 0; i < ch.n_wait; i++) HIPCHK(h, hipStreamWaitEvent(cs, h->seq_done[sched.done_event(ch.wait_last - i)], 0));
    // copy stream: the frames (bytes or floats) and the depths into slots slot ..
    if (u8) HIPCHK(h, hipMemcpyAsync(h->seq_u8.p + (size_t)slot * frame_bytes, (const uint8_t *)frames + (size_t)ch.first * frame_bytes, (size_t)nf * frame_bytes, hipMemcpyHostToDevice, cs));
    else HIPCHK(h, hipMemcpyAsync(img(slot), frames + (size_t)ch.first * 3 * hw, (size_t)nf * 3 * hw * sizeof(float), hipMemcpyHostToDevice, cs));
    if (!gen) HIPCHK(h, hipMemcpyAsync(depth(slot), depths + (size_t)ch.first * hw, (size_t)nf * hw * sizeof(float), hipMemcpyHostToDevice, cs));
    // copy stream: the raw mirror, where somebody reads it.  The frames cross PCIe ONCE: mirrors are device-to-device copies -- of the
    // floats that exist by now (a U8 format's are written by the kernel below, generated depths by the depth stage)
    if (raw_mirror(nm)) {
        if (!u8) HIPCHK(h, hipMemcpyAsync(img(mslot), img(slot), (size_t)nm * 3 * hw * sizeof(float), hipMemcpyDeviceToDevice, cs));
        if (!gen) HIPCHK(h, hipMemcpyAsync(depth(mslot), depth(slot), (size_t)nm * hw * sizeof(float), hipMemcpyDeviceToDevice, cs));
    }
    if (staged) {
        HIPCHK(h, hipEventRecord(h->seq_raw[ch.ev], cs));
        HIPCHK(h, hipStreamWaitEvent(ps, h->seq_raw[ch.ev], 0));
    }
    if (u8) {              // pack stream, first: the chunk's byte slots -> the ring's floats and the raw mirror slots, ONE launch (k_frames_u8, or
        float *mirror = raw_mirror(nm) ? img(mslot) : nullptr;      // k_resize_u8 from camera-size slots)
        const bool hwc = h->seq_fmt == TCSFM_FRAMES_U8_HWC;
        if (resize) HIPCHK(h, launch_resize_u8(ps, *rtab, hwc, true, nf, h->seq_u8.p + (size_t)slot * frame_bytes, img(slot), mirror, mirror ? nm : 0));
        else HIPCHK(h, launch_frames_u8(ps, hwc, nf, h->seq_u8.p + (size_t)slot * 3 * hw, img(slot), mirror, mirror ? nm : 0, hw));
    }
    if (gen) {
        // pack stream: the attached network's clone reads seq_img[slot ..] and writes seq_depth[slot ..], then the depth planes' mirror.
        // Neither the copy stream nor a lane's, so lane 0's windows on h->stream do not hold it up.  The disparity stage is part of it:
        // PLAIN adds a store to the head's launch, POST a mirrored second pass; the store is indexed by the absolute frame.
        void *disp_at = disp_mode == TCSFM_SEQ_DISP_OFF ? nullptr
                        : h->seq_disp_dev.p + (size_t)ch.first * hw * (disp_mode == TCSFM_SEQ_DISP_POST ? sizeof(double) : sizeof(float));
        if ((failed = dn_sequence_depths(h->seq_dn, ps, nf, img(slot), depth(slot), gen_min_disp, gen_max_disp, disp_mode, disp_at, disp_ramp))) return TCSFM_OK;
        if (raw_mirror(nm)) HIPCHK(h, hipMemcpyAsync(depth(mslot), depth(slot), (size_t)nm * hw * sizeof(float), hipMemcpyDeviceToDevice, ps));
    }
    if (scale_on) {
        // pack stream: k_ground + k_median_frames read seq_depth[slot .. slot + nf) (never a mirror slot) and write the stage's own key
        // planes (one chunk's; the next chunk's stage follows on this stream) and the results, by absolute frame
        float *res = h->seq_scale_dev.p + ch.first;
        const size_t cap = h->seq_scale_dev.cap / 3;
        launch_frame_scales(h, ps, nf, depth(slot), h->seq_K.p, 0, h->seq_scale_keys.p, h->seq_cam_height, res, res + cap, (int *)(res + 2 * cap));
    }
    if (use_cache) {           // pack stream: k_frame_pack of the frames that just landed, and of the first nm again into the mirror's packs
        FramePackParams Fp;
        Fp.H = h->H; Fp.W = h->W; Fp.depth_is_disp = o.depth_is_disp;
        Fp.min_disp = o.depth_is_disp ? 1.f / o.max_depth : 0.f; Fp.max_disp = o.depth_is_disp ? 1.f / o.min_depth : 0.f;
        auto pack = [&](int from, int to, int count) {
            Fp.img = img(from); Fp.depth = depth(from);
            Fp.fpack = h->seq_fpack.p + (size_t)to * (h->H + 2) * (h->W + 2); Fp.fdepth = h->seq_fdepth.p + (size_t)to * hw;
            hipLaunchKernelGGL(k_frame_pack, dim3((unsigned)((hw + 255) / 256), count), dim3(256), 0, ps, Fp);
        };
        pack(slot, slot, nf);
        if (nm > 0) pack(slot, mslot, nm);
    }
    HIPCHK(h, hipEventRecord(h->seq_copied[ch.ev], staged ? ps : cs));
    return TCSFM_OK;
}

// Step 5: call ci -- windows c0 .. c0 + nbw - 1 -- on its lane's stream, behind the chunks that hold its frames: the PoseNet loop for the
// initial poses, the refinement (dense: then the maps to the caller), and the call's done-event
int SeqCall::issue_call(const SeqSchedule &sched, long long ci, int c0, int nbw) {
    const int l = (int)(ci % p.L), s0 = c0 % p.R, N = p.N;
    tcsfm_ctx *c = lane[l];
    sched.lane_waits(c0, nbw, waits);
    for (int ev : waits) HIPCHK(h, hipStreamWaitEvent(ls[l], h->seq_copied[ev], 0));
    const float *tg = img(s0 + p.tp), *sr = img(s0), *dt = depth(s0 + p.tp), *ds = depth(s0);       // sources: by position (wo)
    float *p_in = h->seq_pose_in.p + (size_t)c0 * N * 6, *p_out = h->seq_pose_out.p + (size_t)c0 * N * 6;
    if (pn)                // initial poses of these windows: PoseNet -> warp -> PoseNet correction, num_iter times, on the lane
        failed = pose_loop(c, net[l], num_iter, nbw, S, tg, sr, dt, ds, h->seq_K.p, p_in, nullptr, &wo);
    if (!failed && dense) {
        // the call's maps come out stacked [pair index][window]; a small kernel puts them in the caller's per-window order, and ONE
        // copy per call takes them to the host on the lane's stream (asynchronous when the destination is pinned)
        float *tmp = c->seq_dense_tmp.p, *ordered = h->seq_dense.p + (size_t)c0 * N * hw;
        failed = dense_impl(c, &o, N * nbw, nbw, S, CallArgs{tg, sr, dt, ds, h->seq_K.p, p_in, nullptr, p_out, nullptr, tmp, nullptr}, &wo);
        if (!failed) {
            hipLaunchKernelGGL(k_maps_to_window_order, dim3((unsigned)((hw + 255) / 256), N * nbw), dim3(256), 0, ls[l], (const float *)tmp, ordered, nbw, N, (int)hw);
            HIPCHK(h, hipMemcpyAsync(dense_depth_out + (size_t)c0 * N * hw, ordered, (size_t)nbw * N * hw * sizeof(float), hipMemcpyDeviceToHost, ls[l]));
        }
    } else if (!failed) {
        FrameCache fcache = {h->seq_fpack.p, h->seq_fdepth.p, s0, p.tp};
        failed = refine_impl(c, &o, N * nbw, nbw, S, CallArgs{tg, sr, dt, ds, h->seq_K.p, p_in, nullptr, p_out, np == 7 ? h->seq_ls_out.p + (size_t)c0 * N : nullptr, nullptr, nullptr},
                             &wo, use_cache ? &fcache : nullptr);
    }
    if (failed) { if (c != h) h->err = c->err; return TCSFM_OK; }
    HIPCHK(h, hipEventRecord(h->seq_done[sched.done_event(ci)], ls[l]));
    return TCSFM_OK;
}

// Step 6: drain every lane, the copy stream and the pack stream, then the results in one copy each
int SeqCall::drain_fetch() {
    int rc = failed;
    for (hipStream_t s : ls) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess && !rc) { h->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); rc = TCSFM_E_HIP; }
    }
    (void)hipStreamSynchronize(h->seq_copy);
    if (h->seq_pack) (void)hipStreamSynchronize(h->seq_pack);
    if (rc) return rc;
    for (tcsfm_ctx *c : lane)
        if (int rc_ = pending_error(c)) { if (c != h) h->err = c->err; return rc_; }
    auto fetch = [&](float *dst, const float *dev, int per_pair) -> int {     // device (per call, stacked) -> caller (per window)
        if (p.WB == 1) { HIPCHK(h, hipMemcpy(dst, dev, (size_t)p.nwin * p.N * per_pair * sizeof(float), hipMemcpyDeviceToHost)); return TCSFM_OK; }
        stage.resize((size_t)p.nwin * p.N * per_pair);
        HIPCHK(h, hipMemcpy(stage.data(), dev, stage.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int w = 0; w < p.nwin; w++)
            for (int j = 0; j < p.N; j++) memcpy(dst + ((size_t)w * p.N + j) * per_pair, &stage[p.at(w, j) * per_pair], per_pair * sizeof(float));
        return TCSFM_OK;
    };
    if ((rc = fetch(pose_out, h->seq_pose_out.p, 6))) return rc;
    if (pose_init_out && (rc = fetch(pose_init_out, h->seq_pose_in.p, 6))) return rc;
    if (log_scale_out && np == 7 && !dense && (rc = fetch(log_scale_out, h->seq_ls_out.p, 1))) return rc;
    if (scale_on) {       // the frames' scales: one copy per array; kept for tcsfm_sequence_scales
        h->seq_scale_res.resize((size_t)3 * T);
        for (int a = 0; a < 3; a++)
            HIPCHK(h, hipMemcpy(h->seq_scale_res.data() + (size_t)a * T, h->seq_scale_dev.p + (size_t)a * (h->seq_scale_dev.cap / 3), (size_t)T * sizeof(float), hipMemcpyDeviceToHost));
        h->seq_scale_T = T;
    }
    if (disp_mode != TCSFM_SEQ_DISP_OFF) { h->seq_disp_T = T; h->seq_disp_kept = disp_mode; }
    return TCSFM_OK;
}

// The spine: check, reserve, upload, then call by call -- throttle, the chunks that must go up first, the call -- and the drain
int SeqCall::run(const tcsfm_opts *o_in, int ring, int windows_per_call, int target_pos) {
    if (int rc = check(o_in, ring, windows_per_call, target_pos)) return rc;
    DeviceGuard dev_guard(h->device);
    if (int rc = reserve()) return rc;
    if (int rc = upload_small()) return rc;
    SeqSchedule sched(p);
    long long ci = 0;
    for (int c0 = 0; c0 < p.nwin && !failed; c0 += p.WB, ci++) {
        const int nbw = p.nbw(c0), te = sched.throttle_event(ci);
        if (te >= 0) HIPCHK(h, hipEventSynchronize(h->seq_done[te]));
        SeqChunk ch;
        while (!failed && sched.next_chunk(c0, nbw, ch))
            if (int rc = stage_chunk(sched, ch)) return rc;
        if (failed) break;
        if (int rc = issue_call(sched, ci, c0, nbw)) return rc;
        if (!failed) sched.issued(ci, c0, nbw);
    }
    return drain_fetch();
}

int sequence_impl(tcsfm_handle h, const tcsfm_opts *o_in, int T, int S, const float *frames, const float *depths, const float *K,
                  const float *pose_init, tcsfm_posenet *pn, int num_iter, float *pose_init_out, float *pose_out, float *log_scale_out, int ring,
                  int windows_per_call, int target_pos, const char *entry, float *dense_depth_out = nullptr) {
    if (int rc_q = drain_queued(h)) return rc_q;
    if (!h) return TCSFM_E_ARG;
    h->seq_scale_T = 0;                                    // tcsfm_sequence_scales: only a call that succeeds with the stage on leaves results
    h->seq_disp_T = 0;                                     // tcsfm_sequence_disparities: the same rule
    if (!o_in) return fail(h, TCSFM_E_ARG, "opts is NULL");
    SeqCall q{h, entry, T, S, frames, depths, K, pose_init, pn, num_iter, pose_init_out, pose_out, log_scale_out, dense_depth_out};
    return q.run(o_in, ring, windows_per_call, target_pos);
}

}  // namespace

int tcsfm_refine_sequence(tcsfm_handle h, const tcsfm_opts *o, int T, int S, const float *frames, const float *depths, const float *K,
                          const float *pose_init, float *pose_out, float *log_scale_out, int ring, int windows_per_call, int target_pos) {
    if (h && !pose_init) return fail(h, TCSFM_E_ARG, "tcsfm_refine_sequence: NULL input");
    return sequence_impl(h, o, T, S, frames, depths, K, pose_init, nullptr, 0, nullptr, pose_out, log_scale_out, ring, windows_per_call, target_pos, "tcsfm_refine_sequence");
}

int tcsfm_odometry_sequence(tcsfm_handle h, tcsfm_posenet *pn, int num_iter, const tcsfm_opts *o, int T, int S, const float *frames,
                            const float *depths, const float *K, float *pose_init_out, float *pose_out, float *log_scale_out, int ring,
                            int windows_per_call, int target_pos) {
    if (h && !pn) return fail(h, TCSFM_E_ARG, "tcsfm_odometry_sequence: NULL PoseNet");
    return sequence_impl(h, o, T, S, frames, depths, K, nullptr, pn, num_iter, pose_init_out, pose_out, log_scale_out, ring, windows_per_call, target_pos, "tcsfm_odometry_sequence");
}

int tcsfm_refine_dense_sequence(tcsfm_handle h, const tcsfm_opts *o, int T, int S, const float *frames, const float *depths, const float *K,
                                const float *pose_init, float *pose_out, float *depth_out, int ring, int windows_per_call, int target_pos) {
    if (h && (!pose_init || !depth_out)) return fail(h, TCSFM_E_ARG, "tcsfm_refine_dense_sequence: NULL input");
    return sequence_impl(h, o, T, S, frames, depths, K, pose_init, nullptr, 0, nullptr, pose_out, nullptr, ring, windows_per_call, target_pos, "tcsfm_refine_dense_sequence", depth_out);
}

int tcsfm_sequence_frame_format(tcsfm_handle h, int format) {
    if (!h) return TCSFM_E_ARG;
    if (format != TCSFM_FRAMES_F32_CHW && format != TCSFM_FRAMES_U8_CHW && format != TCSFM_FRAMES_U8_HWC)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_frame_format: format must be TCSFM_FRAMES_F32_CHW, TCSFM_FRAMES_U8_CHW or TCSFM_FRAMES_U8_HWC");
    h->seq_fmt = format;
    return TCSFM_OK;
}

int tcsfm_sequence_frame_source(tcsfm_handle h, int src_h, int src_w) {
    if (!h) return TCSFM_E_ARG;
    if (src_h == 0 && src_w == 0) { h->seq_src_h = h->seq_src_w = 0; return TCSFM_OK; }
    if (src_h <= 0 || src_w <= 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_frame_source: src_h and src_w must both be positive, or both 0 (no source size)");
    if (const char *why = resize_refusal(src_h, src_w, h->H, h->W)) return fail(h, TCSFM_E_ARG, (std::string("tcsfm_sequence_frame_source: ") + why).c_str());
    h->seq_src_h = src_h; h->seq_src_w = src_w;
    return TCSFM_OK;
}

int tcsfm_sequence_scale(tcsfm_handle h, float real_cam_height) {
    if (!h) return TCSFM_E_ARG;
    if (!(real_cam_height >= 0.f) || std::isinf(real_cam_height))
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_scale: real_cam_height must be finite and > 0 (stage on) or 0 (off)");
    h->seq_cam_height = real_cam_height;
    return TCSFM_OK;
}

int tcsfm_sequence_scales(tcsfm_handle h, int T, void *scale_out, void *median_out, int *count_out) {
    if (!h) return TCSFM_E_ARG;
    if (!scale_out) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_scales: NULL argument");
    if (h->seq_scale_T == 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_scales: nothing kept (the last sequence call failed or ran with the stage off: tcsfm_sequence_scale)");
    if (T != h->seq_scale_T) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_scales: T differs from the T of the last sequence call");
    const float *r = h->seq_scale_res.data();
    memcpy(scale_out, r, (size_t)T * sizeof(float));
    if (median_out) memcpy(median_out, r + T, (size_t)T * sizeof(float));
    if (count_out) memcpy(count_out, r + 2 * (size_t)T, (size_t)T * sizeof(int));
    return TCSFM_OK;
}

int tcsfm_sequence_disparity(tcsfm_handle h, int mode) {
    if (!h) return TCSFM_E_ARG;
    if (mode != TCSFM_SEQ_DISP_OFF && mode != TCSFM_SEQ_DISP_PLAIN && mode != TCSFM_SEQ_DISP_POST)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_disparity: mode must be TCSFM_SEQ_DISP_OFF, TCSFM_SEQ_DISP_PLAIN or TCSFM_SEQ_DISP_POST");
    h->seq_disp_mode = mode;
    return TCSFM_OK;
}

int tcsfm_sequence_disparities(tcsfm_handle h, int T, int first, int count, void *out, int *mode_out) {
    if (!h) return TCSFM_E_ARG;
    if (!out) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_disparities: NULL argument");
    if (h->seq_disp_T == 0)
        return fail(h, TCSFM_E_ARG, "tcsfm_sequence_disparities: nothing kept (the last sequence call failed or ran with the stage off: tcsfm_sequence_disparity)");
    if (T != h->seq_disp_T) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_disparities: T differs from the T of the last sequence call");
    if (first < 0 || count < 1 || first > T - count) return fail(h, TCSFM_E_ARG, "tcsfm_sequence_disparities: need 0 <= first, count >= 1 and first + count <= T");
    const size_t plane = (size_t)h->H * h->W * (h->seq_disp_kept == TCSFM_SEQ_DISP_POST ? sizeof(double) : sizeof(float));
    DeviceGuard dev_guard(h->device);
    HIPCHK(h, hipMemcpy(out, h->seq_disp_dev.p + (size_t)first * plane, (size_t)count * plane, hipMemcpyDeviceToHost));
    if (mode_out) *mode_out = h->seq_disp_kept;
    return TCSFM_OK;
}
