// gys_devmem.hpp -- the library's only way to allocate device and pinned host memory: DevBuf (device) and PinnedPair (pinned host + device)
// own what they allocate, free it in their destructor and are EMPTY (null pointer, cap 0) after any failed (re)allocation; with them
// the thread's error text (set_err) and HIPCHK.  Needs <hip/hip_runtime.h> and the error codes of gysketch.h, nothing else of the project.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/gysketch.h"

inline thread_local char g_err[512] = "";

inline void set_err(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

#define HIPCHK(expr)                                                                                       \
	do {                                                                                               \
		hipError_t e_ = (expr);                                                                    \
		if (e_ != hipSuccess) {                                                                    \
			set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return GYS_ERR_HIP;                                                                \
		}                                                                                          \
	} while (0)

// An owning device buffer of `cap` elements; reads as a plain T * wherever one is expected.  The destructor frees.
//   alloc(n)         a buffer of max(n, 1) elements, zeroed with hipMemset on the NULL stream unless told otherwise
//   grow(n, s)       keeps a buffer that is large enough; otherwise waits for the stream (a kernel in flight may still read the old
//                    buffer), frees it and allocates anew: the contents are NOT kept
//   grow_keep(n,u,s) the same, but the first `u` elements are kept: the new buffer is allocated first, the old one is freed only after
//                    the copy has finished, and a failure leaves the old buffer and its capacity as they were
template <typename T>
struct DevBuf {
	T *p = nullptr;
	size_t cap = 0;
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		std::swap(p, o.p);
		std::swap(cap, o.cap);
		return *this;
	}
	~DevBuf() { release(); }
	operator T *() const { return p; }
	void release()
	{
		if (p) (void)hipFree(p);
		p = nullptr;
		cap = 0;
	}
	int alloc(size_t n, bool zero = true)
	{
		release();
		n = std::max<size_t>(n, 1);
		HIPCHK(hipMalloc((void **)&p, n * sizeof(T)));
		cap = n;
		if (zero) HIPCHK(hipMemset(p, 0, n * sizeof(T)));
		return GYS_OK;
	}
	int grow(size_t n, hipStream_t stream)
	{
		if (p && cap >= n) return GYS_OK;
		if (p) HIPCHK(hipStreamSynchronize(stream));
		release();
		n = std::max<size_t>(n, 1);
		HIPCHK(hipMalloc((void **)&p, n * sizeof(T)));
		cap = n;
		return GYS_OK;
	}
	int grow_keep(size_t n, size_t used, hipStream_t stream)
	{
		if (p && cap >= n) return GYS_OK;
		DevBuf nb;
		n = std::max<size_t>(n, 1);
		HIPCHK(hipMalloc((void **)&nb.p, n * sizeof(T)));
		nb.cap = n;
		if (p) {
			if (used) HIPCHK(hipMemcpyAsync(nb.p, p, used * sizeof(T), hipMemcpyDeviceToDevice, stream));
			HIPCHK(hipStreamSynchronize(stream)); // (every launch that reads the old buffer is behind us on this stream)
		}
		*this = std::move(nb); // (a swap: nb's destructor frees the old buffer)
		return GYS_OK;
	}
	int upload(const std::vector<T> &v, hipStream_t stream) // (asynchronous: v must outlive the copy)
	{
		const int rc = grow(v.size(), stream);
		if (rc) return rc;
		if (!v.empty()) HIPCHK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
		return GYS_OK;
	}
};

// A pinned host buffer and a device buffer of the same `cap` elements: filled on the host, copied per batch.  grow() keeps a pair that is
// large enough; otherwise it frees both and allocates anew (at least `floor` elements): the contents are NOT kept, and the caller knows
// that nothing in flight reads the old ones.  Both halves or none: a failure leaves the pair empty.  The destructor frees.
template <typename T>
struct PinnedPair {
	T *host = nullptr, *dev = nullptr;
	size_t cap = 0;
	PinnedPair() = default;
	PinnedPair(const PinnedPair &) = delete;
	PinnedPair &operator=(const PinnedPair &) = delete;
	~PinnedPair() { release(); }
	void release()
	{
		if (host) (void)hipHostFree(host);
		if (dev) (void)hipFree(dev);
		host = dev = nullptr;
		cap = 0;
	}
	int grow(size_t n, size_t floor)
	{
		if (n <= cap) return GYS_OK;
		release();
		n = std::max(n, floor);
		const int rc = alloc_halves(n);
		if (rc) release();
		else cap = n;
		return rc;
	}

private:
	int alloc_halves(size_t n)
	{
		HIPCHK(hipHostMalloc((void **)&host, n * sizeof(T), hipHostMallocDefault));
		HIPCHK(hipMalloc((void **)&dev, n * sizeof(T)));
		return GYS_OK;
	}
};
