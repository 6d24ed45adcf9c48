// Host side of the debug readers and of profiling (include/tcsfm.h: tcsfm_debug_check_guards, tcsfm_debug_guard_selftest, tcsfm_debug_trace,
// tcsfm_debug_stamps, tcsfm_profile_*).  Part of tcsfm_api.hip, the library's only translation unit: included after context.h (the
// handle's profile state; ProfScope and take_stamp, which fill it, live there) and device_owned.h (the guard bands).
#pragma once

int tcsfm_debug_check_guards(int *n_allocations, int *n_damaged) {
    if (n_allocations) *n_allocations = -1;
    if (n_damaged) *n_damaged = 0;
    if (!tcguard::on()) return TCSFM_OK;
    if (hipDeviceSynchronize() != hipSuccess) return TCSFM_E_HIP;
    std::lock_guard<std::mutex> lk(tcguard::mtx());
    int bad_allocs = 0;
    for (auto &r : tcguard::recs()) {
        long off = 0;
        const long bad = tcguard::damaged(r, &off);
        if (bad < 0) return TCSFM_E_HIP;
        if (bad > 0) {
            bad_allocs++;
            if (!r.reported)
                fprintf(stderr, "tcsfm guard: allocation of %zu bytes (%s:%d): %ld band bytes overwritten, first at offset %ld of the allocation\n", r.bytes, tcguard::at_file(r), r.line, bad, off);
            r.reported = true;
        }
    }
    if (n_allocations) *n_allocations = (int)tcguard::recs().size();
    if (n_damaged) *n_damaged = bad_allocs;
    return TCSFM_OK;
}

int tcsfm_debug_guard_selftest(int *detected) {
    if (detected) *detected = -1;
    if (!tcguard::on()) return TCSFM_OK;
    DevBuf<char> p, q;
    if (DEV_RESERVE(p, 1000) != hipSuccess) return TCSFM_E_HIP;
    if (hipMemset(p + 1000, 0, 4) != hipSuccess) return TCSFM_E_HIP;      // four bytes past the end
    int found = 0;
    {
        std::lock_guard<std::mutex> lk(tcguard::mtx());
        for (auto &r : tcguard::recs())
            if (r.base + tcguard::kBand == p.p) { long off = 0; found = tcguard::damaged(r, &off) == 4 && off == 1000; r.reported = true; }
    }
    // the check an entry runs over its OWN allocations before it frees them (tcsfm_debug_solve) sees the same damage, and only there
    if (DEV_RESERVE(q, 1000) != hipSuccess) return TCSFM_E_HIP;
    found = found && tcguard::damaged_among({(void *)p.p, (void *)q.p}) == 1 && tcguard::damaged_among({(void *)q.p}) == 0;
    if (detected) *detected = found;
    return TCSFM_OK;
}

int tcsfm_debug_trace(tcsfm_handle h, uint16_t *bits, int64_t bits_capacity, int32_t *decide, int64_t decide_capacity) {
    if (!h) return TCSFM_E_ARG;
    if ((bits && bits_capacity < 1) || (decide && decide_capacity < 1)) return fail(h, TCSFM_E_ARG, "tcsfm_debug_trace: bad capacity");
    h->trace_bits = bits; h->trace_bits_cap = bits ? bits_capacity : 0;
    h->trace_decide = decide; h->trace_decide_cap = decide ? decide_capacity : 0;
    return TCSFM_OK;
}

// diagnostic: copy the k_solve phase stamps to the host (8 values; zeros unless TCSFM_DEBUG_STAMPS was set at create)
int tcsfm_debug_stamps(tcsfm_handle h, long long out[8]) {
    if (!h || !out) return TCSFM_E_ARG;
    memset(out, 0, 8 * sizeof(long long));
    if (!h->dbg_stamps) return TCSFM_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->dbg_stamps, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return TCSFM_OK;
}

int tcsfm_profile_begin(tcsfm_handle h) {
    if (!h) return TCSFM_E_ARG;
    DeviceGuard dev_guard(h->device);
    if (int rc_ = pending_error(h)) return rc_;
    h->stamp_cap = (size_t)4 << 20;         // 4 M workgroup stamps = 64 MB: ~8000 launches of the BASELINE config
    RESERVE(h, h->stamp_buf, h->stamp_cap * 2);
    h->stamp_used = 0;
    h->stamp_launch.clear();
    for (tcsfm_ctx *c : h->lanes)                       // the lanes are bracketed too: their figures are added in profile_end
        if (int rc = tcsfm_profile_begin(c)) { h->err = c->err; return rc; }
    h->profiling = true;
    h->ev_used = 0;
    h->ev_class.clear();
    return TCSFM_OK;
}

int tcsfm_profile_end(tcsfm_handle h, double ms_sum[3], int64_t launches[3]) {
    if (!h || !ms_sum || !launches) return TCSFM_E_ARG;
    h->profiling = false;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) { ms_sum[i] = 0.0; launches[i] = 0; }
    for (size_t k = 0; k < h->ev_class.size(); k++) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev_pool[2 * k], h->ev_pool[2 * k + 1]));
        ms_sum[h->ev_class[k]] += ms;
        launches[h->ev_class[k]]++;
    }
    h->ev_used = 0;
    h->ev_class.clear();
    for (tcsfm_ctx *c : h->lanes) {
        double ms[3]; int64_t n[3];
        if (int rc = tcsfm_profile_end(c, ms, n)) { h->err = c->err; return rc; }
        for (int i = 0; i < 3; i++) { ms_sum[i] += ms[i]; launches[i] += n[i]; }
    }
    return TCSFM_OK;
}

int tcsfm_profile_kernel_time(tcsfm_handle h, double *ms_sum, int64_t *launches) {
    if (!h || !ms_sum || !launches) return TCSFM_E_ARG;
    *ms_sum = 0.0; *launches = 0;
    DeviceGuard dev_guard(h->device);
    if (h->stamp_buf && h->stamp_used > 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<unsigned long long> st(h->stamp_used * 2);
        HIPCHK(h, hipMemcpy(st.data(), h->stamp_buf, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (const auto &l : h->stamp_launch) {     // duration of a launch = latest workgroup end - earliest workgroup start
            unsigned long long t0 = ~0ull, t1 = 0ull;
            for (size_t w = l.first; w < l.first + l.second; w++) { t0 = st[2 * w] < t0 ? st[2 * w] : t0; t1 = st[2 * w + 1] > t1 ? st[2 * w + 1] : t1; }
            if (t1 > t0) { *ms_sum += (double)(t1 - t0) * 1e-5; (*launches)++; }   // 100 MHz ticks -> ms
        }
    }
    for (tcsfm_ctx *c : h->lanes) {
        double ms = 0.0; int64_t n = 0;
        if (int rc = tcsfm_profile_kernel_time(c, &ms, &n)) { h->err = c->err; return rc; }
        *ms_sum += ms; *launches += n;
    }
    return TCSFM_OK;
}

// [start, end] of every stamped launch of the handle and of its lanes, in 100 MHz ticks of the device's s_memrealtime counter
static int profile_intervals(tcsfm_ctx *h, std::vector<std::pair<unsigned long long, unsigned long long>> &out) {
    DeviceGuard dev_guard(h->device);
    if (h->stamp_buf && h->stamp_used > 0) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<unsigned long long> st(h->stamp_used * 2);
        HIPCHK(h, hipMemcpy(st.data(), h->stamp_buf, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (const auto &l : h->stamp_launch) {
            unsigned long long t0 = ~0ull, t1 = 0ull;
            for (size_t w = l.first; w < l.first + l.second; w++) { t0 = st[2 * w] < t0 ? st[2 * w] : t0; t1 = st[2 * w + 1] > t1 ? st[2 * w + 1] : t1; }
            if (t1 > t0) out.push_back({t0, t1});
        }
    }
    for (tcsfm_ctx *c : h->lanes)
        if (int rc = profile_intervals(c, out)) { h->err = c->err; return rc; }
    return TCSFM_OK;
}

int tcsfm_profile_kernel_busy(tcsfm_handle h, double *ms_busy, int64_t *launches) {
    if (!h || !ms_busy || !launches) return TCSFM_E_ARG;
    *ms_busy = 0.0; *launches = 0;
    std::vector<std::pair<unsigned long long, unsigned long long>> iv;
    if (int rc = profile_intervals(h, iv)) return rc;
    std::sort(iv.begin(), iv.end());
    unsigned long long busy = 0, lo = 0, hi = 0;
    bool open = false;
    for (const auto &x : iv) {
        if (open && x.first <= hi) { hi = std::max(hi, x.second); continue; }
        if (open) busy += hi - lo;
        lo = x.first; hi = x.second; open = true;
    }
    if (open) busy += hi - lo;
    *ms_busy = (double)busy * 1e-5;
    *launches = (int64_t)iv.size();
    return TCSFM_OK;
}
