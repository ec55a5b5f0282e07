// owned.h -- move-only owners of the HIP resources the handles hold: device and pinned memory, events, streams, graph executables.
// Host-only, nothing else lives here.  A handle keeps owners as members, its `create` builds into a std::unique_ptr, and `delete` is the whole teardown.
// Every call returns the hipError_t of the one HIP call it makes; the caller wraps it in SVS_HIP so a failure reports the caller's file:line.
// The owners never synchronise: a site that has to drain a stream before a block goes away does so itself (a destructor body runs before the members' destructors).
// comm.hip is NOT converted: its fine-grained / uncached / IPC-mapped memory and the RCCL communicator have lifetimes of their own and stay hand-managed.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <type_traits>
#include <utility>

namespace owned {
// what the owners of this process hold right now (svs_ctx_get_stat: "live_device_bytes", "live_pinned_bytes", "live_sync_objects")
inline std::atomic<long long> g_live_device_bytes{0}, g_live_pinned_bytes{0}, g_live_sync_objects{0};

// memory that the CALLER of the C API owns (svs_malloc / svs_free): passed through and deliberately NOT counted -- svs_free is not told a size, and blocks a
// caller still holds would keep the counters above from returning exactly to an earlier reading
inline hipError_t caller_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t caller_free(void *p) { return hipFree(p); }

template <class T, bool Pinned>
class Buf {
  T *p_ = nullptr;
  size_t bytes_ = 0;
  static constexpr size_t elem() { if constexpr (std::is_void_v<T>) return 1; else return sizeof(T); }
  static std::atomic<long long> &live() { return Pinned ? g_live_pinned_bytes : g_live_device_bytes; }

 public:
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
  ~Buf() { reset(); }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t bytes() const { return bytes_; }
  void reset() {
    if (!p_) return;
    if (Pinned) (void)hipHostFree(p_); else (void)hipFree(p_);
    live() -= (long long)bytes_;
    p_ = nullptr; bytes_ = 0;
  }
  // a fresh block (whatever was held goes first); `view`: where the kernel parameter struct wants the raw pointer
  hipError_t alloc_bytes(size_t bytes, T **view = nullptr) {
    reset();
    void *p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e == hipSuccess) { p_ = static_cast<T *>(p); bytes_ = bytes; live() += (long long)bytes; }
    if (view) *view = p_;
    return e;
  }
  hipError_t alloc(size_t count, T **view = nullptr) { return alloc_bytes(count * elem(), view); }
  // grow-only; the slack is the caller's: a block of >= need_bytes is kept, anything else (no block at all included) is replaced by one of want_bytes.
  // reserve: free, then allocate -- contents undefined.  reserve_keep: allocate, copy keep_bytes device-to-device, free the old block.
  hipError_t reserve(size_t need_bytes, size_t want_bytes) { return p_ && bytes_ >= need_bytes ? hipSuccess : alloc_bytes(want_bytes); }
  hipError_t reserve_keep(size_t need_bytes, size_t want_bytes, size_t keep_bytes) {
    static_assert(!Pinned, "reserve_keep copies device-to-device");
    if (p_ && bytes_ >= need_bytes) return hipSuccess;
    Buf n;
    hipError_t e = n.alloc_bytes(want_bytes);
    if (e == hipSuccess && p_ && keep_bytes) e = hipMemcpy(n.p_, p_, keep_bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) *this = std::move(n);
    return e;
  }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// one owner per kind of synchronisation object; H: the handle, Destroy: the call that ends it
template <class H, hipError_t (*Destroy)(H)>
class SyncObj {
 protected:
  H h_ = nullptr;
  hipError_t adopt(hipError_t e) { if (e == hipSuccess) ++g_live_sync_objects; else h_ = nullptr; return e; }

 public:
  SyncObj() = default;
  SyncObj(SyncObj &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  SyncObj &operator=(SyncObj &&o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); } return *this; }
  ~SyncObj() { reset(); }
  H get() const { return h_; }
  operator H() const { return h_; }
  void reset() {
    if (!h_) return;
    (void)Destroy(h_); --g_live_sync_objects;
    h_ = nullptr;
  }
};
struct Event : SyncObj<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) { reset(); return adopt(hipEventCreateWithFlags(&h_, flags)); }
};
// a stream the library made.  A stream it was GIVEN (svs_ctx_create with the caller's stream) is held as a plain hipStream_t beside an empty owner: never destroyed
struct Stream : SyncObj<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) { reset(); return adopt(hipStreamCreateWithFlags(&h_, flags)); }
  hipError_t create(unsigned flags, int priority) { reset(); return adopt(hipStreamCreateWithPriority(&h_, flags, priority)); }
};
struct GraphExec : SyncObj<hipGraphExec_t, hipGraphExecDestroy> {
  hipError_t instantiate(hipGraph_t g) { reset(); return adopt(hipGraphInstantiate(&h_, g, nullptr, nullptr, 0)); }
};
}  // namespace owned
using owned::DevBuf;
using owned::PinnedBuf;
