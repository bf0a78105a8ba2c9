// bf_host.h — the host plumbing around every launch, shared by bf_handle (bf_api.cpp), bf_lua
// (bf_lua.hip) and bf_bank (bf_bank.hip), and in part by bf_multi.cpp: the common state, the error
// formatter and check macro, the device and stream-order guards, the call scope that holds them
// with the mutex, the key-status report and the per-kernel profile.  Host only.
#pragma once
#include "bf_internal.h"

#include <mutex>
#include <optional>
#include <string>
#include <vector>

struct BfProfAcc { std::string name; double ms; uint64_t launches; };

// What bf_handle, bf_lua and bf_bank derive from.  The handle types are opaque in bfhip.h.
struct BfHostCore {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;   // *_last_error(h); written only with mu held
    // cross-stream ordering (StreamOrder): the event after the handle's last device work
    hipEvent_t order_ev = nullptr;
    hipStream_t order_stream = nullptr;
    bool order_valid = false;
    // per-kernel timing (prof_begin): event sets awaiting harvest, recycled sets, totals
    bool profile = false;
    std::vector<BfMarks> prof_pending, prof_free;
    std::vector<BfProfAcc> prof_acc;
};

// The one error formatter: the message goes to c->err, or without a handle to *create_err (the
// family's thread-local string, what its *_last_error(NULL) returns).  Returns code.
int bf_set_err(BfHostCore* c, std::string* create_err, int code, const char* fmt, ...);
// HIPCHK's failure on a live handle: "<expr> failed: <hip error>", out of memory as BF_ENOMEM.
int bf_hip_fail(BfHostCore* c, hipError_t e, const char* expr);

#define HIPCHK(h, expr)                                        \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return bf_hip_fail((h), e_, #expr); \
    } while (0)

// Makes a device current for the duration of a call.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Orders one handle's device work across streams: work arriving on a different stream than the
// previous call's first waits for that call's last launch (hipStreamWaitEvent, no host sync).
// Calls on one stream pay only an event record.
struct StreamOrder {
    BfHostCore* c;
    hipStream_t s;
    StreamOrder(BfHostCore* c_, hipStream_t s_) : c(c_), s(s_) {
        if (c->order_valid && c->order_stream != s) (void)hipStreamWaitEvent(s, c->order_ev, 0);
    }
    ~StreamOrder() {
        if (c->order_ev && hipEventRecord(c->order_ev, s) == hipSuccess) {
            c->order_valid = true;
            c->order_stream = s;
        }
    }
    StreamOrder(const StreamOrder&) = delete;
    StreamOrder& operator=(const StreamOrder&) = delete;
};

// One entry point's hold on a handle.  Constructed first, so the mutex is held before anything
// writes c->err; the argument refusals follow; then device() or open() before the first HIP
// call.  Destruction runs in reverse: the stream-order event is recorded, the device restored,
// the mutex released.
struct CallScope {
    BfHostCore* c;
    std::lock_guard<std::mutex> lk;
    std::optional<DeviceGuard> dg;
    std::optional<StreamOrder> so;
    hipStream_t s = nullptr;   // the call's stream, after open()
    explicit CallScope(BfHostCore* c_) : c(c_), lk(c_->mu) {}
    // The handle's device made current; BF_EDEVICE when that fails.
    int device();
    // device(), then stream s_ ordered after the handle's last work.
    int open(hipStream_t s_);
};

// Device pointer + 16-byte alignment bias for the kernels.
inline const uint8_t* align_keys(const uint8_t* p, uint64_t* bias) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    *bias = a & 15u;
    return reinterpret_cast<const uint8_t*>(a & ~(uintptr_t)15);
}

// The key-status word (BfGeom::key_status, pinned host memory the kernels write when a key's
// offsets fail bfdev::key_ok): reported once, as BF_EINVAL, by the next call on the handle.
int take_key_status(BfHostCore* c, uint32_t* h_key_status);

// Per-kernel timing: an event set per launch (nullptr unless c->profile), harvested into
// c->prof_acc by prof_harvest; prof_read harvests and fills the *_profile_read output arrays.
BfMarks* prof_begin(BfHostCore* c, hipStream_t s);
int prof_harvest(BfHostCore* c);
int prof_read(BfHostCore* c, char* names, double* total_ms, uint64_t* launches, uint32_t cap, uint32_t* n_out,
              uint32_t reset);
// Destroys the events of every set, harvested or not (the handle's destroy).
void prof_destroy(BfHostCore* c);
