// host_rt.cpp -- the device and pinned-host pools of the C ABI's host layer, the buffers
// built on them, and the small helpers of host_rt.hpp.
#include "host_rt.hpp"

#include <map>

namespace fstamd::host {

thread_local HostProf* t_prof = nullptr;
thread_local LaunchStats t_last_stats;

int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  return dev;
}

bool fault_inject(const char* site) {
  const char* e = std::getenv("FSTAMD_FAULT_INJECT");
  return e && std::strcmp(e, site) == 0;
}

bool read_file(const char* path, long max_bytes, std::vector<char>* data) {
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return false;
  bool ok = std::fseek(fp, 0, SEEK_END) == 0;
  const long sz = ok ? std::ftell(fp) : -1;
  ok = sz >= 0 && sz <= max_bytes;
  if (ok) {
    data->resize((size_t)sz);
    std::rewind(fp);
    ok = sz == 0 || std::fread(data->data(), 1, (size_t)sz, fp) == (size_t)sz;
  }
  std::fclose(fp);
  return ok;
}

bool d2h(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  return bytes == 0 ||
         hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
}

bool read_u64(void* dst, const void* dev_src, hipStream_t stream) {
  return hipMemcpyAsync(dst, dev_src, 8, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipStreamSynchronize(stream) == hipSuccess;
}

// Device buffers of the batch calls come from a per-process pool of power-of-two blocks:
// hipMalloc / hipFree of tens of MB per call (inputs, arena, CSR results) cost up to
// ~20 ms of host time a call, and hipFree synchronises the device.  Every DevBuf user
// synchronises before the buffer goes back, so a block is never reused while a kernel
// still runs on it.  Blocks beyond kPoolMax bytes held are freed instead; fst_teardown
// empties the pool.
// Blocks above kPoolMaxBlock (multi-GB path arenas) are never cached: they would hold HBM
// the dense replay sizes its waves from (hipMemGetInfo).  A failed hipMalloc releases the
// device's cached blocks and retries once, so cached blocks of other size classes can never
// turn into an FST_OOM.
namespace {
constexpr size_t kPoolMax = 8ull << 30;
constexpr size_t kPoolMaxBlock = 1ull << 30;
struct BufPool {
  std::mutex mu;
  std::multimap<std::pair<int, size_t>, void*> free;
  size_t held = 0;
};
BufPool& buf_pool() {
  static BufPool* p = new BufPool;  // never destroyed: DevBufs may outlive static teardown
  return *p;
}
}  // namespace

void pool_release(int dev) {
  BufPool& P = buf_pool();
  // the blocks leave the pool under the lock; hipFree (it synchronises the device) runs
  // after it, so other threads' DevBuf allocations never wait for a running kernel here
  std::vector<std::pair<int, void*>> drop;
  {
    std::lock_guard<std::mutex> g(P.mu);
    for (auto it = P.free.begin(); it != P.free.end();) {
      if (dev >= 0 && it->first.first != dev) {
        ++it;
        continue;
      }
      drop.emplace_back(it->first.first, it->second);
      P.held -= it->first.second;
      it = P.free.erase(it);
    }
  }
  if (drop.empty()) return;
  int cur = 0;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  for (auto& [d, p] : drop) {
    (void)hipSetDevice(d);
    (void)hipFree(p);
  }
  if (have_cur) (void)hipSetDevice(cur);
}

DevBuf::DevBuf(size_t n) {
  cls = 4096;
  while (cls < n) cls <<= 1;
  if (hipGetDevice(&dev) != hipSuccess) return;
  BufPool& P = buf_pool();
  {
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.free.find({dev, cls});
    if (it != P.free.end()) {
      p = it->second;
      P.free.erase(it);
      P.held -= cls;
      return;
    }
  }
  if (hipMalloc(&p, cls) == hipSuccess) return;
  p = nullptr;
  (void)hipGetLastError();
  pool_release(dev);  // cached blocks of other classes back to the device, then retry
  if (hipMalloc(&p, cls) == hipSuccess) return;
  (void)hipGetLastError();
  DeviceEngine::trim_idle(dev);  // and the idle engines' workspaces
  (void)hipSetDevice(dev);
  if (hipMalloc(&p, cls) != hipSuccess) p = nullptr;
}

DevBuf::~DevBuf() {
  if (!p) return;
  BufPool& P = buf_pool();
  std::lock_guard<std::mutex> g(P.mu);
  if (cls <= kPoolMaxBlock && P.held + cls <= kPoolMax) {
    P.free.insert({{dev, cls}, p});
    P.held += cls;
  } else {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(dev);
    (void)hipFree(p);
    (void)hipSetDevice(cur);
  }
}

// Result arrays of the batch entries (FstBatchResult) come from a pool of pinned host
// blocks: the device writes them by DMA, with no staging through the runtime's bounce
// buffers and no page faults on freshly malloc'd pages every call (config 4 returns ~50 MB
// of paths per 64 K utterances).  fst_batch_result_free gives them back; beyond
// kPinPoolMax held they are freed.  A failed pinned allocation falls back to malloc.
namespace {
constexpr size_t kPinPoolMax = 4ull << 30;
struct PinPool {
  std::mutex mu;
  std::multimap<size_t, void*> free;       // size class -> pinned block
  std::map<void*, std::pair<size_t, bool>> live;  // block -> (size class, pinned)
  size_t held = 0;
};
PinPool& pin_pool() {
  static PinPool* p = new PinPool;  // never destroyed: results may outlive static teardown
  return *p;
}
}  // namespace

void* pin_alloc(size_t n) {
  size_t c = 4096;
  while (c < n) c <<= 1;
  PinPool& P = pin_pool();
  std::lock_guard<std::mutex> g(P.mu);
  auto it = P.free.find(c);
  if (it != P.free.end()) {
    void* p = it->second;
    P.free.erase(it);
    P.held -= c;
    P.live[p] = {c, true};
    return p;
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, c, hipHostMallocDefault) == hipSuccess && p) {
    P.live[p] = {c, true};
    return p;
  }
  p = std::malloc(c);
  if (p) P.live[p] = {c, false};
  return p;
}
void pin_release(void* p) {
  if (!p) return;
  PinPool& P = pin_pool();
  std::lock_guard<std::mutex> g(P.mu);
  auto it = P.live.find(p);
  if (it == P.live.end()) return;  // not ours (never happens through the API)
  const size_t c = it->second.first;
  const bool pinned = it->second.second;
  P.live.erase(it);
  if (!pinned) {
    std::free(p);
  } else if (P.held + c <= kPinPoolMax) {
    P.free.insert({c, p});
    P.held += c;
  } else {
    (void)hipHostFree(p);
  }
}
bool pin_is_pinned(const void* p) {
  PinPool& P = pin_pool();
  std::lock_guard<std::mutex> g(P.mu);
  auto it = P.live.find(const_cast<void*>(p));
  return it != P.live.end() && it->second.second;
}
void pin_pool_clear() {
  PinPool& P = pin_pool();
  std::lock_guard<std::mutex> g(P.mu);
  for (auto& kv : P.free) (void)hipHostFree(kv.second);
  P.free.clear();
  P.held = 0;
}

DevOut::DevOut(uint32_t num, uint64_t arc_cap)
    : status(num * 4ull), len(num * 4ull), off(num * 8ull), fin(num * 8ull), il(arc_cap * 4),
      ol(arc_cap * 4), w(arc_cap * 8), cursor(8) {
  v.status = (int32_t*)status.p;
  v.path_len = (uint32_t*)len.p;
  v.path_off = (uint64_t*)off.p;
  v.final_w = (double*)fin.p;
  v.out_il = (uint32_t*)il.p;
  v.out_ol = (uint32_t*)ol.p;
  v.out_w = (double*)w.p;
  v.arc_cap = arc_cap;
  v.cursor = (unsigned long long*)cursor.p;
  v.work = nullptr;
}

bool DevOut::download(uint32_t num, HostPaths* h, hipStream_t stream) const {
  h->status.resize(num);
  h->len.resize(num);
  h->off.resize(num);
  h->fin.resize(num);
  unsigned long long used = 0;
  if (!read_u64(&used, cursor.p, stream)) return false;
  used = std::min<unsigned long long>(used, v.arc_cap);
  h->il.resize(used);
  h->ol.resize(used);
  h->w.resize(used);
  // HostPaths is pinned: the copies run asynchronously, one synchronisation for all
  return d2h(h->status.data(), status.p, num * 4ull, stream) &&
         d2h(h->len.data(), len.p, num * 4ull, stream) &&
         d2h(h->off.data(), off.p, num * 8ull, stream) &&
         d2h(h->fin.data(), fin.p, num * 8ull, stream) &&
         d2h(h->il.data(), il.p, used * 4, stream) && d2h(h->ol.data(), ol.p, used * 4, stream) &&
         d2h(h->w.data(), w.p, used * 8, stream) && hipStreamSynchronize(stream) == hipSuccess;
}

}  // namespace fstamd::host

namespace fstamd {  // the pools for device_engine.hip (HostLattice, the dense replay's budget)
void* pin_host_alloc(size_t bytes) { return host::pin_alloc(bytes); }
void pin_host_release(void* p) { host::pin_release(p); }
void device_pool_release(int dev) { host::pool_release(dev); }
}  // namespace fstamd
