// The owners of gyeeta_amd/csrc/gys_devmem.hpp (DevBuf, PinnedPair) without a GPU: compiled by g++ with AddressSanitizer and UBSan over
// the CPU stand-in of <hip/hip_runtime.h> (tests/cpp/kemu) and a fake allocator for the nine HIP entry points the header uses, backed
// by malloc / free.  The fake counts live blocks, logs every call in order and can fail the k-th allocation from now.
// Exit status 0 and "devmem ok" when every case holds; LeakSanitizer has the last word on anything the counters missed.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>

// ---- the fake HIP runtime
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
typedef struct fake_stream_t *hipStream_t;
constexpr unsigned hipHostMallocDefault = 0;

namespace fake {
struct Ev {
	char what; // 'a' device alloc, 'h' pinned alloc, 'f' device free, 'g' pinned free, 'c' copy, 's' stream sync, 'z' memset
	void *p, *src;
};
std::map<void *, std::pair<size_t, bool>> live; // block -> (bytes, pinned)
std::vector<Ev> log;
int fail_in = 0; // > 0: the fail_in-th allocation from now fails
int bad = 0;     // frees of something that is not a live block of that kind

hipError_t alloc(void **p, size_t bytes, bool pinned)
{
	if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;
	*p = malloc(bytes ? bytes : 1);
	memset(*p, 0xA5, bytes); // (what an allocation that is not cleared holds)
	live[*p] = {bytes, pinned};
	log.push_back({pinned ? 'h' : 'a', *p, nullptr});
	return hipSuccess;
}
hipError_t release(void *p, bool pinned)
{
	auto it = live.find(p);
	if (it == live.end() || it->second.second != pinned) {
		++bad;
		return hipErrorInvalidValue;
	}
	live.erase(it);
	log.push_back({pinned ? 'g' : 'f', p, nullptr});
	free(p);
	return hipSuccess;
}
size_t count(char what, const void *p = nullptr)
{
	size_t n = 0;
	for (const Ev &e : log) n += e.what == what && (!p || e.p == p);
	return n;
}
long index_of(char what, const void *p)
{
	for (size_t i = 0; i < log.size(); ++i)
		if (log[i].what == what && log[i].p == p) return (long)i;
	return -1;
}
} // namespace fake

hipError_t hipMalloc(void **p, size_t bytes) { return fake::alloc(p, bytes, false); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake::alloc(p, bytes, true); }
hipError_t hipFree(void *p) { return fake::release(p, false); }
hipError_t hipHostFree(void *p) { return fake::release(p, true); }
hipError_t hipMemset(void *p, int v, size_t bytes)
{
	memset(p, v, bytes);
	fake::log.push_back({'z', p, nullptr});
	return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t)
{
	memcpy(dst, src, bytes);
	fake::log.push_back({'c', dst, (void *)src});
	return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
	fake::log.push_back({'s', nullptr, nullptr});
	return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }
const char *hipGetErrorName(hipError_t e) { return e == hipSuccess ? "hipSuccess" : e == hipErrorOutOfMemory ? "hipErrorOutOfMemory" : "hipErrorInvalidValue"; }

#include "../../gyeeta_amd/csrc/gys_devmem.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                          \
	do {                                                                 \
		if (!(cond)) {                                               \
			printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++g_fail;                                            \
		}                                                            \
	} while (0)

static void fresh()
{
	CHECK(fake::live.empty());
	CHECK(fake::bad == 0);
	fake::log.clear();
	fake::fail_in = 0;
}

static bool all_bytes(const void *p, size_t n, uint8_t v)
{
	for (size_t i = 0; i < n; ++i)
		if (((const uint8_t *)p)[i] != v) return false;
	return true;
}

// grow, then grow larger: one live block, the first freed once; a grow that fits keeps the block
static void case_grow()
{
	fresh();
	{
		DevBuf<uint32_t> b;
		CHECK(b.grow(100, nullptr) == GYS_OK && b.p && b.cap == 100);
		uint32_t *first = b.p;
		CHECK(b.grow(50, nullptr) == GYS_OK && b.p == first && b.cap == 100);
		CHECK(fake::count('a') == 1 && fake::count('s') == 0);
		CHECK(b.grow(1000, nullptr) == GYS_OK && b.cap == 1000);
		CHECK(fake::live.size() == 1 && fake::live.count(b.p) && fake::live[b.p].first == 4000);
		CHECK(fake::count('f', first) == 1 && fake::count('f') == 1);
		CHECK(fake::count('s') == 1 && fake::index_of('s', nullptr) < fake::index_of('f', first)); // waits for the stream, then frees
		uint32_t *q = b; // reads as a plain pointer
		CHECK(q == b.p && b + 3 == b.p + 3 && &b[5] == b.p + 5 && (bool)b);
		DevBuf<uint32_t> z;
		CHECK(z.grow(0, nullptr) == GYS_OK && z.p && z.cap == 1); // (a count of 0 becomes 1)
	}
	CHECK(fake::live.empty() && fake::count('f') == 3);
}

static void case_alloc()
{
	fresh();
	{
		DevBuf<uint64_t> a, b, z;
		CHECK(a.alloc(33) == GYS_OK && a.cap == 33 && all_bytes(a.p, 33 * 8, 0));
		CHECK(b.alloc(33, false) == GYS_OK && b.cap == 33 && all_bytes(b.p, 33 * 8, 0xA5));
		CHECK(fake::count('z') == 1 && fake::count('z', a.p) == 1);
		CHECK(z.alloc(0) == GYS_OK && z.p && z.cap == 1 && fake::live[z.p].first == 8);
		fake::fail_in = 1;
		DevBuf<uint64_t> f;
		CHECK(f.alloc(10) == GYS_ERR_HIP && !f.p && f.cap == 0 && strstr(g_err, "out of memory"));
	}
	CHECK(fake::live.empty());
}

// a grow whose allocation fails leaves the buffer EMPTY (not dangling with a capacity that says "large enough")
static void case_grow_fails()
{
	fresh();
	{
		DevBuf<uint8_t> b;
		CHECK(b.grow(64, nullptr) == GYS_OK);
		void *first = b.p;
		fake::fail_in = 1;
		CHECK(b.grow(1 << 20, nullptr) == GYS_ERR_HIP);
		CHECK(b.p == nullptr && b.cap == 0 && fake::live.empty() && fake::count('f', first) == 1);
		CHECK(b.grow(1 << 20, nullptr) == GYS_OK && b.p && b.cap == (1u << 20));
		memset(b.p, 1, b.cap); // (the whole capacity is there)
		CHECK(fake::live.size() == 1);
	}
	CHECK(fake::live.empty() && fake::count('a') == 2 && fake::count('f') == 2 && fake::bad == 0);
}

static void case_pinned_pair()
{
	fresh();
	{
		PinnedPair<uint8_t> pp;
		CHECK(pp.grow(10, 4096) == GYS_OK && pp.host && pp.dev && pp.cap == 4096 && fake::live.size() == 2);
		CHECK(fake::live[pp.host].second && !fake::live[pp.dev].second);
		uint8_t *h = pp.host;
		CHECK(pp.grow(4096, 4096) == GYS_OK && pp.host == h); // fits: kept
		fake::fail_in = 2; // the device half
		CHECK(pp.grow(8192, 4096) == GYS_ERR_HIP);
		CHECK(!pp.host && !pp.dev && pp.cap == 0 && fake::live.empty());
		fake::fail_in = 1; // the host half
		CHECK(pp.grow(8192, 4096) == GYS_ERR_HIP && !pp.host && !pp.dev && pp.cap == 0 && fake::live.empty());
		CHECK(pp.grow(8192, 4096) == GYS_OK && pp.cap == 8192 && fake::live.size() == 2);
	}
	CHECK(fake::live.empty() && fake::bad == 0 && fake::count('h') == fake::count('g') && fake::count('a') == fake::count('f'));
}

static void case_grow_keep()
{
	fresh();
	{
		DevBuf<uint32_t> b;
		CHECK(b.grow_keep(4096, 0, nullptr) == GYS_OK && b.cap == 4096 && fake::count('c') == 0); // first use: nothing to keep
		for (uint32_t i = 0; i < 3000; ++i) b.p[i] = i * 7u + 1u;
		uint32_t *old = b.p;
		CHECK(b.grow_keep(4000, 3000, nullptr) == GYS_OK && b.p == old); // fits
		CHECK(b.grow_keep(8192, 3000, nullptr) == GYS_OK && b.p != old && b.cap == 8192 && fake::live.size() == 1);
		bool same = true;
		for (uint32_t i = 0; i < 3000; ++i) same = same && b.p[i] == i * 7u + 1u;
		CHECK(same);
		// new block, copy out of the old one, the stream drained, and only then the old block freed
		const long ia = fake::index_of('a', b.p), ic = fake::index_of('c', b.p), ifr = fake::index_of('f', old);
		CHECK(ia >= 0 && ia < ic && ic < ifr && fake::log[ic].src == old);
		bool synced = false;
		for (long i = ic + 1; i < ifr; ++i) synced = synced || fake::log[i].what == 's';
		CHECK(synced);
		// a failure leaves the old block, its contents and its capacity
		old = b.p;
		fake::fail_in = 1;
		CHECK(b.grow_keep(1 << 16, 3000, nullptr) == GYS_ERR_HIP && b.p == old && b.cap == 8192 && fake::live.size() == 1);
		CHECK(b.p[2999] == 2999u * 7u + 1u);
	}
	CHECK(fake::live.empty() && fake::bad == 0);
}

static void case_swap_move()
{
	fresh();
	{
		DevBuf<uint32_t> a, b;
		CHECK(a.alloc(10) == GYS_OK && b.alloc(20) == GYS_OK);
		uint32_t *pa = a.p, *pb = b.p;
		std::swap(a, b);
		CHECK(a.p == pb && a.cap == 20 && b.p == pa && b.cap == 10 && fake::live.size() == 2 && fake::count('f') == 0);
		DevBuf<uint32_t> c2;
		CHECK(c2.alloc(30) == GYS_OK);
		uint32_t *pc = c2.p;
		a = std::move(c2); // a's old block goes with c2
		CHECK(a.p == pc && a.cap == 30 && fake::live.size() == 3);
		DevBuf<uint32_t> d(std::move(b));
		CHECK(d.p == pa && !b.p && b.cap == 0);
	}
	CHECK(fake::live.empty() && fake::bad == 0 && fake::count('a') == 3 && fake::count('f') == 3);
}

// the shape of the wire front end's reservation: seven arrays that grow together and a slot count that holds only when all seven stand
struct Wire {
	uint64_t slots_cap = 0;
	DevBuf<uint32_t> jump[2], cnt, rank, bsums;
	DevBuf<uint8_t> mark, flags;
	int reserve(uint64_t nslots)
	{
		if (nslots + 1 > slots_cap) {
			const uint64_t cap = (std::max<uint64_t>(nslots + 1, 1u << 10) + 255) / 256 * 256;
			slots_cap = 0;
			int rc = GYS_OK;
			for (DevBuf<uint32_t> *b : {&jump[0], &jump[1], &cnt, &rank})
				if (!rc) rc = b->grow(cap, nullptr);
			if (!rc) rc = bsums.grow(cap / 256 + 2, nullptr);
			if (!rc) rc = mark.grow(cap, nullptr);
			if (!rc) rc = flags.grow(cap, nullptr);
			if (rc) return rc;
			slots_cap = cap;
		}
		return GYS_OK;
	}
	size_t owners() const { return !!jump[0].p + !!jump[1].p + !!cnt.p + !!rank.p + !!bsums.p + !!mark.p + !!flags.p; }
};

static void case_seven_arrays()
{
	for (int from_small = 0; from_small < 2; ++from_small)
		for (int k = 1; k <= 8; ++k) { // (k = 8: no allocation fails)
			fresh();
			{
				Wire w;
				if (from_small) CHECK(w.reserve(100) == GYS_OK && w.owners() == 7 && fake::live.size() == 7);
				fake::fail_in = k;
				const int rc = w.reserve(5000);
				CHECK(rc == (k <= 7 ? GYS_ERR_HIP : GYS_OK));
				CHECK(fake::live.size() == w.owners());
				CHECK(rc ? w.slots_cap == 0 : w.slots_cap >= 5001);
				CHECK(w.owners() == (size_t)(from_small || k == 8 ? (k <= 7 ? 6 : 7) : k - 1));
				fake::fail_in = 0;
				CHECK(w.reserve(200) == GYS_OK && w.owners() == 7 && fake::live.size() == 7 && w.slots_cap >= 201);
				for (DevBuf<uint32_t> *b : {&w.jump[0], &w.jump[1], &w.cnt, &w.rank}) CHECK(b->cap >= w.slots_cap);
				CHECK(w.bsums.cap >= w.slots_cap / 256 + 2 && w.mark.cap >= w.slots_cap && w.flags.cap >= w.slots_cap);
			}
			CHECK(fake::live.empty() && fake::bad == 0);
		}
}

int main()
{
	case_grow();
	case_alloc();
	case_grow_fails();
	case_pinned_pair();
	case_grow_keep();
	case_swap_move();
	case_seven_arrays();
	fresh();
	if (g_fail) {
		printf("%d checks failed\n", g_fail);
		return 1;
	}
	printf("devmem ok\n");
	return 0;
}
