// DevBuf<T>: the one owner of a device allocation.  Host-only C++: no HIP header is included, memory is reached through the two
// functions declared below, which the including translation unit defines (cdae_hip.hip: hipMalloc / hipFree; tests/native/
// dev_buf_cpu.cpp: malloc / free with a live-block counter).
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>

namespace cdae { namespace mem {
// 0 = success; on failure the function has already recorded the error (fail()) and *p is left as it was
int acquire(void** p, size_t bytes);
int release(void* p);
} }  // namespace cdae::mem

// p holds at least cap elements (ensure(): cap units of `per` elements, the `per` of the calls that grew it).  drop() is the only way
// either member is cleared, so a freed buffer can never keep a capacity that ensure() would believe — and a null p means "not
// allocated for this data set" wherever the pointer doubles as a flag.  Move-only; the destructor releases.
template <class T> struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { (void)drop(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
    return *this;
  }
  ~DevBuf() { (void)drop(); }
  // grow-only: nothing happens at cap >= n
  int ensure(size_t n, size_t per = 1) {
    if (cap >= n) return 0;
    if (int rc = drop()) return rc;
    if (int rc = acquire_elems(n * per)) return rc;
    cap = n;
    return 0;
  }
  // exactly n elements (at least one, so that the pointer is non-null): what set_interactions sizes once per data set
  int alloc(size_t n) {
    if (int rc = drop()) return rc;
    if (int rc = acquire_elems(n)) return rc;
    cap = n;
    return 0;
  }
  int drop() {                  // both members are cleared whatever release answers
    T* const old = p;
    p = nullptr; cap = 0;
    return old ? cdae::mem::release(old) : 0;
  }
  operator T*() const { return p; }

 private:
  int acquire_elems(size_t n) {
    void* q = nullptr;
    if (int rc = cdae::mem::acquire(&q, std::max<size_t>(n, 1) * sizeof(T))) return rc;
    p = static_cast<T*>(q);
    return 0;
  }
};
