// mnav_buf.h -- owners of the host code's device memory, pinned host memory, streams, events and graph executables.
// Host only: kernels and kernel-argument structs take raw pointers (get(), or the implicit conversion).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace mnav {

// One allocation of device memory (Pinned = false) or pinned host memory (Pinned = true), freed with its owner.
// Move-only; an owner must never have static storage duration (its destructor would run after the HIP runtime's).
template <class T, bool Pinned>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buf& operator=(Buf&& o) noexcept
  {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
    return *this;
  }
  ~Buf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t bytes() const { return bytes_; }

  void reset()
  {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; bytes_ = 0;
  }
  // frees the old allocation first; on failure the buffer is left empty
  hipError_t alloc(size_t bytes)
  {
    reset();
    void* p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p); bytes_ = bytes;
    return hipSuccess;
  }
  // n elements from the host (none when `host` is null) on `stream`, into a buffer with 64 bytes of tail slack: clamped
  // vector loads may touch element 0 of an empty tile.  A buffer of the same size is kept (cost re-uploads).
  hipError_t upload(hipStream_t stream, const T* host, size_t n)
  {
    const size_t want = sizeof(T) * (n ? n : 1) + 64;
    if (!p_ || bytes_ != want) {
      const hipError_t e = alloc(want);
      if (e != hipSuccess) return e;
    }
    return (n && host) ? hipMemcpyAsync(p_, host, sizeof(T) * n, hipMemcpyHostToDevice, stream) : hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// Allocates a group of buffers that one guard stands for (buffer, bytes, buffer, bytes, ...) in argument order: all of
// them, or -- on a failure part-way -- none, so that the next call starts from empty.
inline hipError_t alloc_group() { return hipSuccess; }
template <class B, class... Rest>
hipError_t alloc_group(B& b, size_t bytes, Rest&&... rest)
{
  hipError_t e = b.alloc(bytes);
  if (e == hipSuccess) e = alloc_group(std::forward<Rest>(rest)...);
  if (e != hipSuccess) b.reset();
  return e;
}

// One runtime handle, destroyed with its owner.  out() destroys the old handle and hands the slot to a create call.
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept
  {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
    return *this;
  }
  ~Handle() { reset(); }

  operator H() const { return h_; }
  H* out() { reset(); return &h_; }
  void reset()
  {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 private:
  H h_ = nullptr;
};

using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace mnav
