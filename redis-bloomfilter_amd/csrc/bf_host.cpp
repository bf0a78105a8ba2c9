// bf_host.cpp — the shared host core of bf_handle, bf_lua and bf_bank (bf_host.h).
#include "bf_host.h"
#include "bfhip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

int bf_set_err(BfHostCore* c, std::string* create_err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else *create_err = buf;
    return code;
}

int bf_hip_fail(BfHostCore* c, hipError_t e, const char* expr) {
    return bf_set_err(c, nullptr, e == hipErrorOutOfMemory ? BF_ENOMEM : BF_EDEVICE, "%s failed: %s", expr,
                      hipGetErrorString(e));
}

int CallScope::device() {
    if (!dg) dg.emplace(c->device);
    return dg->ok ? BF_OK : bf_set_err(c, nullptr, BF_EDEVICE, "hipSetDevice(%d) failed", c->device);
}

int CallScope::open(hipStream_t s_) {
    if (int rc = device()) return rc;
    s = s_;
    so.emplace(c, s_);
    return BF_OK;
}

int take_key_status(BfHostCore* c, uint32_t* h_key_status) {
    if (!h_key_status || __atomic_load_n(h_key_status, __ATOMIC_ACQUIRE) == 0u) return BF_OK;
    __atomic_store_n(h_key_status, 0u, __ATOMIC_RELEASE);
    return bf_set_err(c, nullptr, BF_EINVAL,
                      "an earlier call's key offsets were inconsistent (offsets must be non-decreasing "
                      "and every key below 2 GiB): those keys were hashed as empty strings");
}

BfMarks* prof_begin(BfHostCore* c, hipStream_t s) {
    if (!c->profile) return nullptr;
    BfMarks mk{};
    if (!c->prof_free.empty()) {
        mk = c->prof_free.back();
        c->prof_free.pop_back();
    } else {
        for (hipEvent_t& e : mk.ev)
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
    }
    mk.used = 0;
    if (hipEventRecord(mk.ev[0], s) != hipSuccess) {
        c->prof_free.push_back(mk);
        return nullptr;
    }
    c->prof_pending.push_back(mk);
    return &c->prof_pending.back();
}

int prof_harvest(BfHostCore* c) {
    for (BfMarks& mk : c->prof_pending) {
        if (mk.used > 0) HIPCHK(c, hipEventSynchronize(mk.ev[mk.used]));
        for (int i = 0; i < mk.used; ++i) {
            float ms = 0.f;
            HIPCHK(c, hipEventElapsedTime(&ms, mk.ev[i], mk.ev[i + 1]));
            auto it = std::find_if(c->prof_acc.begin(), c->prof_acc.end(),
                                   [&](const BfProfAcc& a) { return a.name == mk.names[i]; });
            if (it == c->prof_acc.end()) c->prof_acc.push_back({mk.names[i], (double)ms, 1});
            else { it->ms += ms; it->launches += 1; }
        }
        c->prof_free.push_back(mk);
    }
    c->prof_pending.clear();
    return BF_OK;
}

int prof_read(BfHostCore* c, char* names, double* total_ms, uint64_t* launches, uint32_t cap, uint32_t* n_out,
              uint32_t reset) {
    int rc = prof_harvest(c);
    if (rc) return rc;
    *n_out = (uint32_t)c->prof_acc.size();
    for (uint32_t i = 0; i < cap && i < c->prof_acc.size(); ++i) {
        const BfProfAcc& a = c->prof_acc[i];
        if (names) snprintf(names + (size_t)i * BF_PROFILE_NAME_LEN, BF_PROFILE_NAME_LEN, "%s", a.name.c_str());
        if (total_ms) total_ms[i] = a.ms;
        if (launches) launches[i] = a.launches;
    }
    if (reset) c->prof_acc.clear();
    return BF_OK;
}

void prof_destroy(BfHostCore* c) {
    for (std::vector<BfMarks>* v : {&c->prof_pending, &c->prof_free})
        for (BfMarks& mk : *v)
            for (hipEvent_t e : mk.ev)
                if (e) (void)hipEventDestroy(e);
}
