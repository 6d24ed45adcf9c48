// Host side of the device optimiser (optim_kernel.h): the tensor and work tables built at create, the per-step table staged through a
// ring of pinned slots, the arenas of the moments and of the snapshot, and the tcsfm_optim_* entry points.  Part of tcsfm_api.hip, the
// library's only translation unit: included after context.h (the owners of device_owned.h, fail_alloc) and the networks'
// host headers.
#pragma once

struct tcsfm_optim {
    tcsfm_ctx *h = nullptr;
    int kind = 0, n = 0, nwork = 0;
    std::vector<OptTensor> T;            // host mirror of the device tensor table
    std::vector<long long> step;         // per tensor: optimiser steps taken (torch's state['step'])
    DevBuf<OptTensor> T_dev;
    DevBuf<OptWork> work_dev;
    DevBuf<float> moments, snap;                   // arenas: [exp_avg | exp_avg_sq] (Adam only), the snapshot (allocated by the first snapshot)
    size_t arena = 0;                    // floats of one arena: every tensor at its parameter's 16-byte phase
    bool has_snapshot = false;
    // Per-step tables (gradient pointers and scalars) go host -> pinned slot -> device slot -> kernel, all on the stream.  A slot is
    // rewritten only once the step that used it has finished (its event), so steps issued back to back each keep their own table.
    static constexpr int kRing = 4;
    PinnedBuf<OptStep> stage_host;       // [kRing][n]
    DevBuf<OptStep> stage_dev;
    Events ring_ev;                      // kRing of them
    bool ring_used[kRing] = {};
    unsigned long long seq = 0;
};

namespace {
int opt_blocks(int nwork) { return std::min(nwork, OPT_MAX_BLOCKS); }

// copy the host tensor table to the device (create, and the first snapshot, which adds the snapshot pointers)
int opt_upload_tensors(tcsfm_optim *o) {
    tcsfm_ctx *h = o->h;
    HIPCHK(h, hipStreamSynchronize(h->stream));       // an earlier step may be reading the table
    HIPCHK(h, hipMemcpy(o->T_dev, o->T.data(), o->T.size() * sizeof(OptTensor), hipMemcpyHostToDevice));
    return TCSFM_OK;
}

template <int KIND>
void opt_launch(tcsfm_optim *o, const OptStep *steps, const OptScalars &C) {
    if (!o->nwork) return;
    hipLaunchKernelGGL((k_optim<KIND>), dim3(opt_blocks(o->nwork)), dim3(OPT_THREADS), 0, o->h->stream, (const OptTensor *)o->T_dev, steps,
                       (const OptWork *)o->work_dev, o->nwork, C);
}
}  // namespace

// ---- entry points (include/tcsfm.h) ---------------------------------------------------------------------------------------------
void tcsfm_optim_destroy(tcsfm_optim *o) {
    if (!o) return;
    DeviceGuard dev_guard(o->h->device);
    // the stream may still run a step that reads the tables and writes the arenas
    if (o->h->stream) (void)hipStreamSynchronize(o->h->stream);
    for (size_t k = 0; k < o->ring_ev.size(); k++) (void)hipEventSynchronize(o->ring_ev[k]);
    delete o;
}

int tcsfm_optim_create(tcsfm_handle h, int kind, int n, float *const params[], const int64_t numel[], tcsfm_optim **out) {
    if (!h || !out) return TCSFM_E_ARG;
    *out = nullptr;
    if (kind != TCSFM_OPTIM_ADAM && kind != TCSFM_OPTIM_SGD) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: unknown kind (TCSFM_OPTIM_ADAM or TCSFM_OPTIM_SGD)");
    if (n < 1 || !params || !numel) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: needs at least one parameter tensor");
    long long nwork = 0;
    size_t arena = 0;
    std::vector<OptTensor> T(n);
    std::vector<size_t> at(n);
    for (int i = 0; i < n; i++) {
        if (numel[i] < 0) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: negative numel");
        if (numel[i] > 0 && !params[i]) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: NULL parameter pointer");
        if (((uintptr_t)params[i] & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: parameter pointer is not 4-byte aligned");
        const size_t phase = ((uintptr_t)params[i] >> 2) & 3;
        at[i] = (arena + 3) / 4 * 4 + phase;                  // the arenas are 256-byte aligned: this offset has the parameter's phase
        arena = at[i] + (size_t)numel[i];
        T[i] = {params[i], nullptr, nullptr, nullptr, (long long)numel[i]};
        nwork += ((long long)numel[i] + (long long)phase + OPT_CHUNK - 1) / OPT_CHUNK;
    }
    if (nwork > 0x7fffffffLL) return fail(h, TCSFM_E_ARG, "tcsfm_optim_create: too many elements for one optimiser");
    {   // the tensors are updated in place by every step: two of them sharing memory would be stepped twice
        ArgRanges a;
        for (int i = 0; i < n; i++) a.out("params", params[i], (size_t)numel[i] * sizeof(float), i);
        if (int rc = check_overlap(h, "tcsfm_optim_create", a)) return rc;
    }
    if (int rc = drain_queued(h)) return rc;
    DeviceGuard dev_guard(h->device);
    tcsfm_optim *o = new tcsfm_optim();
    o->h = h; o->kind = kind; o->n = n; o->nwork = (int)nwork; o->arena = (std::max<size_t>(arena, 4) + 3) / 4 * 4;     // (a multiple of four floats: the second moment's half keeps the phases)
    o->step.assign(n, 0);
    std::vector<OptWork> work;
    work.reserve((size_t)nwork);
    for (int i = 0; i < n; i++) {
        const long long phase = ((uintptr_t)params[i] >> 2) & 3, chunks = ((long long)numel[i] + phase + OPT_CHUNK - 1) / OPT_CHUNK;
        for (long long c = 0; c < chunks; c++) work.push_back({i, (int)c});
    }
    hipError_t e = DEV_RESERVE(o->T_dev, n);
    if (e == hipSuccess) e = DEV_RESERVE(o->work_dev, std::max<size_t>(work.size(), 1));
    if (e == hipSuccess) e = DEV_RESERVE(o->stage_dev, (size_t)tcsfm_optim::kRing * n);
    if (e == hipSuccess) e = o->stage_host.create((size_t)tcsfm_optim::kRing * n, hipHostMallocDefault);
    if (e == hipSuccess && kind == TCSFM_OPTIM_ADAM) {
        e = DEV_RESERVE(o->moments, 2 * o->arena);
        if (e == hipSuccess) e = hipMemsetAsync(o->moments, 0, 2 * o->arena * sizeof(float), h->stream);
        for (int i = 0; i < n; i++) { T[i].m = o->moments + at[i]; T[i].v = o->moments + o->arena + at[i]; }
    }
    if (e == hipSuccess) e = o->ring_ev.grow(tcsfm_optim::kRing);
    if (e == hipSuccess && !work.empty()) e = hipMemcpy(o->work_dev, work.data(), work.size() * sizeof(OptWork), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->T_dev, T.data(), n * sizeof(OptTensor), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);       // the arenas are zero before the handle's stream can change
    o->T = std::move(T);
    if (e != hipSuccess) {
        tcsfm_optim_destroy(o);
        return fail_alloc(h, e, "tcsfm_optim_create: allocation failed");
    }
    *out = o;
    return TCSFM_OK;
}

int tcsfm_optim_step(tcsfm_optim *o, const float *const grads[], const double lr[], double beta1, double beta2, double eps) {
    if (!o) return TCSFM_E_ARG;
    tcsfm_ctx *h = o->h;
    if (!grads || !lr) return fail(h, TCSFM_E_ARG, "tcsfm_optim_step: grads and lr are tables of n entries");
    for (int i = 0; i < o->n; i++)
        if (((uintptr_t)grads[i] & 3) != 0) return fail(h, TCSFM_E_ARG, "tcsfm_optim_step: gradient pointer is not 4-byte aligned");
    {   // a gradient that lies on a parameter (its own or another tensor's) is read while the step rewrites it
        ArgRanges a;
        for (int i = 0; i < o->n; i++) {
            a.in("grads", grads[i], (size_t)o->T[i].numel * sizeof(float), i);
            if (grads[i]) a.out("params", o->T[i].p, (size_t)o->T[i].numel * sizeof(float), i);
        }
        if (int rc = check_overlap(h, "tcsfm_optim_step", a)) return rc;
    }
    if (int rc = drain_queued(h)) return rc;
    DeviceGuard dev_guard(h->device);
    const int slot = (int)(o->seq % tcsfm_optim::kRing);
    if (o->ring_used[slot]) HIPCHK(h, hipEventSynchronize(o->ring_ev[slot]));      // (only with kRing steps in flight)
    OptStep *host = o->stage_host + (size_t)slot * o->n, *dev = o->stage_dev + (size_t)slot * o->n;
    bool any = false;
    for (int i = 0; i < o->n; i++) {
        host[i] = {grads[i], 0.f, 1.f};
        if (!grads[i]) continue;                      // torch: p.grad is None -> no update, state['step'] does not move
        const long long t = ++o->step[i];
        any = any || o->T[i].numel > 0;
        if (o->kind == TCSFM_OPTIM_ADAM) {
            const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
            host[i].a = (float)(lr[i] / bc1);
            host[i].b = (float)sqrt(bc2);
        } else {
            host[i].a = (float)lr[i];
        }
    }
    if (!any) return TCSFM_OK;
    o->seq++;
    OptScalars C;
    C.one_m_b1 = (float)(1.0 - beta1); C.b2 = (float)beta2; C.one_m_b2 = (float)(1.0 - beta2); C.eps = (float)eps;
    HIPCHK(h, hipMemcpyAsync(dev, host, o->n * sizeof(OptStep), hipMemcpyHostToDevice, h->stream));
    if (o->kind == TCSFM_OPTIM_ADAM) opt_launch<OPT_ADAM>(o, dev, C);
    else opt_launch<OPT_SGD>(o, dev, C);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(o->ring_ev[slot], h->stream));
    o->ring_used[slot] = true;
    return TCSFM_OK;
}

int tcsfm_optim_snapshot(tcsfm_optim *o) {
    if (!o) return TCSFM_E_ARG;
    tcsfm_ctx *h = o->h;
    if (int rc = drain_queued(h)) return rc;
    DeviceGuard dev_guard(h->device);
    if (!o->snap) {
        hipError_t e = DEV_RESERVE(o->snap, o->arena);
        if (e == hipSuccess) e = hipMemsetAsync(o->snap, 0, o->arena * sizeof(float), h->stream);
        if (e != hipSuccess) return fail_alloc(h, e, "tcsfm_optim_snapshot: allocation failed");
        size_t at = 0;
        for (int i = 0; i < o->n; i++) {              // the offsets of tcsfm_optim_create
            at = (at + 3) / 4 * 4 + (((uintptr_t)o->T[i].p >> 2) & 3);
            o->T[i].snap = o->snap + at;
            at += (size_t)o->T[i].numel;
        }
        if (int rc = opt_upload_tensors(o)) return rc;
    }
    opt_launch<OPT_SNAPSHOT>(o, nullptr, OptScalars{});
    HIPCHK(h, hipGetLastError());
    o->has_snapshot = true;
    return TCSFM_OK;
}

int tcsfm_optim_restore(tcsfm_optim *o) {
    if (!o) return TCSFM_E_ARG;
    tcsfm_ctx *h = o->h;
    if (!o->has_snapshot) return fail(h, TCSFM_E_ARG, "tcsfm_optim_restore: no snapshot was taken (tcsfm_optim_snapshot)");
    if (int rc = drain_queued(h)) return rc;
    DeviceGuard dev_guard(h->device);
    opt_launch<OPT_RESTORE>(o, nullptr, OptScalars{});
    HIPCHK(h, hipGetLastError());
    if (o->moments) HIPCHK(h, hipMemsetAsync(o->moments, 0, 2 * o->arena * sizeof(float), h->stream));
    std::fill(o->step.begin(), o->step.end(), 0LL);
    return TCSFM_OK;
}

int tcsfm_optim_get_state(tcsfm_optim *o, int i, float *exp_avg_out, float *exp_avg_sq_out, int64_t *step_out) {
    if (!o) return TCSFM_E_ARG;
    tcsfm_ctx *h = o->h;
    if (i < 0 || i >= o->n) return fail(h, TCSFM_E_ARG, "tcsfm_optim_get_state: tensor index out of range");
    if (o->kind != TCSFM_OPTIM_ADAM && (exp_avg_out || exp_avg_sq_out)) return fail(h, TCSFM_E_ARG, "tcsfm_optim_get_state: an SGD optimiser keeps no moments (pass NULL)");
    if (step_out) *step_out = (int64_t)o->step[i];
    const size_t bytes = (size_t)o->T[i].numel * sizeof(float);
    if (!bytes || !(exp_avg_out || exp_avg_sq_out)) return TCSFM_OK;
    {
        ArgRanges a;
        a.out("exp_avg_out", exp_avg_out, bytes); a.out("exp_avg_sq_out", exp_avg_sq_out, bytes);
        if (int rc = check_overlap(h, "tcsfm_optim_get_state", a)) return rc;
    }
    DeviceGuard dev_guard(h->device);
    if (exp_avg_out) HIPCHK(h, hipMemcpyAsync(exp_avg_out, o->T[i].m, bytes, hipMemcpyDefault, h->stream));
    if (exp_avg_sq_out) HIPCHK(h, hipMemcpyAsync(exp_avg_sq_out, o->T[i].v, bytes, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return TCSFM_OK;
}
