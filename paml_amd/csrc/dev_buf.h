// dev_buf.h — the two owners of device resources: a grow-only device buffer and an event.  Both free what they hold in their destructor,
// move and do not copy, so a struct of them needs no destructor of its own.  Used by the engine (engine_state.h) and by the stand-alone
// entries that have no engine (engine_rell.hip, engine_compress.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

namespace paml_amd {

// bytes of device memory that DevBuf objects of this process hold now (paml_amd_debug_device_bytes)
inline std::atomic<long long> dev_buf_bytes{0};

template <typename T>
struct DevBuf {
   T *p = nullptr;
   size_t cap = 0;
   DevBuf() = default;
   DevBuf(const DevBuf &) = delete;
   DevBuf &operator=(const DevBuf &) = delete;
   DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
   DevBuf &operator=(DevBuf &&o) noexcept
   {
      if (this != &o) {
         release();
         p = o.p; cap = o.cap;
         o.p = nullptr; o.cap = 0;
      }
      return *this;
   }
   ~DevBuf() { release(); }
   hipError_t ensure(size_t n)
   {
      if (n <= cap) return hipSuccess;
      release();
      hipError_t e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T));
      if (e != hipSuccess) { p = nullptr; return e; }
      cap = n;
      dev_buf_bytes += (long long)bytes();
      return e;
   }
   void release()
   {
      if (p) {
         dev_buf_bytes -= (long long)bytes();
         (void)hipFree(p);
      }
      p = nullptr;
      cap = 0;
   }
   size_t bytes() const { return p ? std::max<size_t>(cap, 1) * sizeof(T) : 0; }      // (ensure(0) still allocates one element)
};

// An event, created by the first ensure() and destroyed with its owner; reads as the hipEvent_t it holds (null before ensure).
struct DevEvent {
   hipEvent_t ev = nullptr;
   DevEvent() = default;
   DevEvent(const DevEvent &) = delete;
   DevEvent &operator=(const DevEvent &) = delete;
   DevEvent(DevEvent &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
   DevEvent &operator=(DevEvent &&o) noexcept
   {
      if (this != &o) {
         release();
         ev = o.ev;
         o.ev = nullptr;
      }
      return *this;
   }
   ~DevEvent() { release(); }
   hipError_t ensure(unsigned flags = hipEventDefault) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
   void release()
   {
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
   }
   operator hipEvent_t() const { return ev; }
};

}  // namespace paml_amd
