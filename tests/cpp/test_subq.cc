// The submission queues and the staging ring of gyeeta_amd/csrc/gys_subq.hpp without a GPU: a stand-alone program, compiled by g++ once with
// ThreadSanitizer and once with AddressSanitizer + UBSan (tests/test_subq_cpu.py) over the CPU stand-in of <hip/hip_runtime.h>
// (tests/cpp/kemu) and a fake of the host entry points the header uses.  The fake is a DEVICE THREAD that executes each stream's
// operations in order and honours hipStreamWaitEvent across streams; the test can pause and release it, fail the k-th allocation, the
// k-th launch, and put the k-th recorded event into an error state.  A copy and a launch run on that thread WHEN REACHED, not at
// enqueue: a batch or slot that is reused before its `done` event has fired shows as wrong contents and as a data race.
// The properties checked are the sentences of the protocol comment in gys_subq.hpp; the letters (a) .. (k) below name them.
// Usage: test_subq SEED.  Exit status 0 and "subq ok" when every case holds.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <set>

// ---- the fake HIP runtime
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorNotReady = 600, hipErrorLaunchFailure = 719 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToDevice = 3 };
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2;

struct fake_event_t {
	std::atomic<uint64_t> recorded{0}, done{0}; // records enqueued / executed
	std::atomic<int> err{0};                    // the last executed record left the event in an error state
};
typedef fake_event_t *hipEvent_t;

struct FakeOp {
	enum { COPY, RECORD, WAIT, CALL } what;
	void *dst = nullptr;
	const void *src = nullptr;
	size_t n = 0;
	hipEvent_t ev = nullptr;
	uint64_t seq = 0;
	bool bad = false;
	std::function<void()> fn;
};
struct fake_stream_t {
	std::deque<FakeOp> ops;
};
typedef fake_stream_t *hipStream_t;

namespace fake {
std::mutex m; // the streams' queues, the counters below
std::condition_variable cv;
std::vector<hipStream_t> streams;
bool paused = false, quit = false;
uint64_t pending = 0; // operations enqueued and not yet executed
int fail_alloc_in = 0, fail_record_in = 0; // > 0: the k-th from now fails / ends in an error state
long live_blocks = 0, live_events = 0, bad_frees = 0;
std::set<void *> blocks;

void enqueue(hipStream_t s, FakeOp op)
{
	std::lock_guard<std::mutex> g(m);
	s->ops.push_back(std::move(op));
	++pending;
	cv.notify_all();
}
// the engine's side of a launch: `fn` runs on the device thread when the stream reaches it
void launch(hipStream_t s, std::function<void()> fn)
{
	FakeOp op;
	op.what = FakeOp::CALL;
	op.fn = std::move(fn);
	enqueue(s, std::move(op));
}
bool runnable(const FakeOp &op) { return op.what != FakeOp::WAIT || op.ev->done.load(std::memory_order_acquire) >= op.seq; }
void device_thread()
{
	std::unique_lock<std::mutex> lk(m);
	for (;;) {
		hipStream_t pick = nullptr;
		cv.wait(lk, [&] {
			if (quit) return true;
			if (paused) return false;
			for (hipStream_t s : streams)
				if (!s->ops.empty() && runnable(s->ops.front())) {
					pick = s;
					return true;
				}
			return false;
		});
		if (quit) return;
		FakeOp op = std::move(pick->ops.front());
		pick->ops.pop_front();
		lk.unlock();
		if (op.what == FakeOp::COPY) memcpy(op.dst, op.src, op.n);
		else if (op.what == FakeOp::CALL) op.fn();
		else if (op.what == FakeOp::RECORD) {
			op.ev->err.store(op.bad, std::memory_order_relaxed);
			op.ev->done.store(op.seq, std::memory_order_release);
		}
		lk.lock();
		--pending;
		cv.notify_all();
	}
}
void pause()
{
	std::lock_guard<std::mutex> g(m);
	paused = true;
}
void resume()
{
	std::lock_guard<std::mutex> g(m);
	paused = false;
	cv.notify_all();
}
void sync() // everything enqueued so far has been executed
{
	std::unique_lock<std::mutex> lk(m);
	cv.wait(lk, [] { return pending == 0; });
}
hipStream_t stream_create()
{
	std::lock_guard<std::mutex> g(m);
	streams.push_back(new fake_stream_t);
	return streams.back();
}
void streams_destroy()
{
	std::lock_guard<std::mutex> g(m);
	for (hipStream_t s : streams) delete s;
	streams.clear();
}
hipError_t alloc(void **p, size_t bytes)
{
	std::lock_guard<std::mutex> g(m);
	if (fail_alloc_in > 0 && --fail_alloc_in == 0) return hipErrorOutOfMemory;
	*p = malloc(bytes ? bytes : 1);
	blocks.insert(*p);
	++live_blocks;
	return hipSuccess;
}
hipError_t release(void *p)
{
	{
		std::lock_guard<std::mutex> g(m);
		if (!blocks.erase(p)) {
			++bad_frees;
			return hipErrorInvalidValue;
		}
		--live_blocks;
	}
	free(p);
	return hipSuccess;
}
} // namespace fake

hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char *hipGetErrorString(hipError_t e)
{
	return e == hipSuccess ? "success" : e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorNotReady ? "not ready" : e == hipErrorLaunchFailure ? "launch failure" : "invalid value";
}
hipError_t hipMalloc(void **p, size_t bytes) { return fake::alloc(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake::alloc(p, bytes); }
hipError_t hipFree(void *p) { return fake::release(p); }
hipError_t hipHostFree(void *p) { return fake::release(p); }
hipError_t hipStreamSynchronize(hipStream_t) // (gys_devmem.hpp names it; nothing in gys_subq.hpp reaches it)
{
	fake::sync();
	return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s)
{
	FakeOp op;
	op.what = FakeOp::COPY;
	op.dst = dst, op.src = src, op.n = bytes;
	fake::enqueue(s, std::move(op));
	return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned)
{
	*ev = new fake_event_t;
	std::lock_guard<std::mutex> g(fake::m);
	++fake::live_events;
	return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev)
{
	delete ev;
	std::lock_guard<std::mutex> g(fake::m);
	--fake::live_events;
	return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s)
{
	FakeOp op;
	op.what = FakeOp::RECORD;
	op.ev = ev;
	std::lock_guard<std::mutex> g(fake::m);
	op.seq = ev->recorded.load(std::memory_order_relaxed) + 1;
	ev->recorded.store(op.seq, std::memory_order_release);
	op.bad = fake::fail_record_in > 0 && --fake::fail_record_in == 0;
	s->ops.push_back(std::move(op));
	++fake::pending;
	fake::cv.notify_all();
	return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t ev, unsigned)
{
	FakeOp op;
	op.what = FakeOp::WAIT;
	op.ev = ev;
	op.seq = ev->recorded.load(std::memory_order_acquire); // (the record the stream waits for: the last one enqueued)
	fake::enqueue(s, std::move(op));
	return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t ev) // (an event that was never recorded is complete, as in HIP)
{
	if (ev->done.load(std::memory_order_acquire) < ev->recorded.load(std::memory_order_acquire)) return hipErrorNotReady;
	return ev->err.load(std::memory_order_relaxed) ? hipErrorLaunchFailure : hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev)
{
	const uint64_t want = ev->recorded.load(std::memory_order_acquire);
	while (ev->done.load(std::memory_order_acquire) < want) std::this_thread::sleep_for(std::chrono::microseconds(50));
	return ev->err.load(std::memory_order_relaxed) ? hipErrorLaunchFailure : hipSuccess;
}

#include "../../gyeeta_amd/csrc/gys_subq.hpp"

using namespace gys;
using Clock = std::chrono::steady_clock;

static std::atomic<int> g_fail{0};
#define CHECK(cond)                                                          \
	do {                                                                 \
		if (!(cond)) {                                               \
			if (g_fail++ < 40) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
		}                                                            \
	} while (0)

// every wait of the test runs against this clock: a phase that does not end inside its bound fails the test (a lost wake-up, a drained
// free list and a flusher that never comes are hangs, not wrong answers)
static std::atomic<int64_t> g_deadline_ms{0};
static std::atomic<const char *> g_phase{""};
static int64_t now_ms() { return std::chrono::duration_cast<std::chrono::milliseconds>(Clock::now().time_since_epoch()).count(); }
static void phase(const char *name, int secs)
{
	g_phase = name;
	g_deadline_ms.store(now_ms() + secs * 1000ll);
}
static void watchdog()
{
	for (;;) {
		std::this_thread::sleep_for(std::chrono::milliseconds(20));
		const int64_t d = g_deadline_ms.load();
		if (d < 0) return;
		if (d && now_ms() > d) {
			printf("FAILED: \"%s\" did not end inside its bound\n", g_phase.load());
			fflush(stdout);
			_exit(3);
		}
	}
}
template <class F>
static bool wait_for(F cond, int ms)
{
	const int64_t end = now_ms() + ms;
	while (!cond()) {
		if (now_ms() > end) return false;
		std::this_thread::sleep_for(std::chrono::microseconds(200));
	}
	return true;
}

// ---- what the callers send.  A response event is [call id + 1, index, 16 random bytes]; a record is [call id + 1, index, 0 .. 3 random
// words], so a call's bytes are not always a multiple of 8.  Everything a launch sees names the call it came from.
struct Call {
	SubQ::Kind kind;
	uint32_t host, thread, seq, n;
	std::vector<uint8_t> data;
	std::vector<uint32_t> offs;
	int rc = -1;
	int found = 0, sub = -1;
};

// what a launch was given (on the host: kind, counts, segments, the device pointer; on the device thread, when reached: the bytes)
struct Submission {
	SubQ::Kind kind;
	const uint8_t *dev;
	uint64_t fill;
	uint32_t nrec;
	std::vector<gys_resp_seg> segs;
	std::vector<uint8_t> bytes;
	std::vector<uint32_t> offs, hosts;
};

constexpr uint32_t NHOSTS = 32, NTHREADS = 16;

struct Rig {
	IngestEnv env;
	SubQ sq[3];
	StageRing ring;
	std::mutex enq_mu;
	std::mutex log_mu;
	std::vector<std::unique_ptr<Submission>> log[3]; // in launch order == order on the engine stream
	std::atomic<int> inside[3] = {}, inside_any{0};
	std::atomic<int> fail_launch_in{0};
	std::atomic<int> launch_us{0}; // the device takes this long over a submission
	std::vector<Call> calls;

	explicit Rig(uint64_t max_batch_events = 4096)
	{
		env.device = 0;
		env.stream = fake::stream_create();
		env.copy_stream = fake::stream_create();
		env.enq_mu = &enq_mu;
		env.max_batch_events = max_batch_events;
		env.launch = [this](SubQ::Kind kind, const uint8_t *dev, uint64_t fill, uint32_t nrec, const std::vector<gys_resp_seg> &segs) {
			return launch(kind, dev, fill, nrec, segs);
		};
		for (SubQ::Kind k : {SubQ::RESP, SubQ::CONN, SubQ::LSTATE}) subq_init(env, sq[k], k);
	}
	~Rig()
	{
		ingest_teardown(sq, 3, ring, [] { fake::sync(); });
		fake::streams_destroy();
	}
	int launch(SubQ::Kind kind, const uint8_t *dev, uint64_t fill, uint32_t nrec, const std::vector<gys_resp_seg> &segs)
	{
		CHECK(inside[kind].fetch_add(1) == 0); // never entered twice at once for one queue
		CHECK(inside_any.fetch_add(1) == 0);   // ... nor for two: enq_mu is held
		int rc = GYS_OK;
		int k = fail_launch_in.load();
		if (k > 0 && fail_launch_in.fetch_sub(1) == 1) {
			set_err("launch refused");
			rc = GYS_ERR_HIP;
		} else {
			auto sub = std::make_unique<Submission>();
			Submission *s = sub.get();
			s->kind = kind, s->dev = dev, s->fill = fill, s->nrec = nrec, s->segs = segs;
			const SubQ &q = sq[kind];
			const int us = launch_us.load();
			fake::launch(env.stream, [s, &q, us] {
				if (s->kind == SubQ::RESP) {
					s->bytes.assign(s->dev, s->dev + s->fill * 24);
				} else {
					s->bytes.assign(s->dev, s->dev + s->fill);
					const uint32_t *o = (const uint32_t *)(s->dev + q.cap);
					s->offs.assign(o, o + s->nrec);
					if (s->kind == SubQ::LSTATE) s->hosts.assign(o + q.cap_recs, o + q.cap_recs + s->nrec);
				}
				if (us) std::this_thread::sleep_for(std::chrono::microseconds(us));
			});
			std::lock_guard<std::mutex> g(log_mu);
			log[kind].push_back(std::move(sub));
		}
		inside_any.fetch_sub(1);
		inside[kind].fetch_sub(1);
		return rc;
	}
	size_t launched(SubQ::Kind k)
	{
		std::lock_guard<std::mutex> g(log_mu);
		return log[k].size();
	}
	uint64_t submissions(SubQ::Kind k)
	{
		std::lock_guard<std::mutex> g(sq[k].mu);
		return sq[k].submissions;
	}
	uint64_t pending(SubQ::Kind k) // (as gys_resp_queue_pending counts it)
	{
		SubQ &q = sq[k];
		std::lock_guard<std::mutex> g(q.mu);
		uint64_t n = q.open >= 0 ? q.b[q.open].fill : 0;
		for (int bi : q.sealed) n += q.b[bi].fill;
		return n;
	}
	size_t add_call(std::mt19937_64 &rng, SubQ::Kind kind, uint32_t host, uint32_t thread, uint32_t seq, uint32_t n, uint32_t fixed_words = ~0u)
	{
		Call c;
		c.kind = kind, c.host = host, c.thread = thread, c.seq = seq, c.n = n;
		const uint32_t id = (uint32_t)calls.size() + 1;
		for (uint32_t i = 0; i < n; ++i) {
			const uint32_t extra = kind == SubQ::RESP ? 4 : fixed_words != ~0u ? fixed_words : (uint32_t)(rng() % 4);
			if (kind != SubQ::RESP) c.offs.push_back((uint32_t)c.data.size());
			std::vector<uint32_t> w = {id, i};
			for (uint32_t e = 0; e < extra; ++e) w.push_back((uint32_t)rng());
			c.data.insert(c.data.end(), (uint8_t *)w.data(), (uint8_t *)(w.data() + w.size()));
		}
		calls.push_back(std::move(c));
		return calls.size() - 1;
	}
	int send(size_t ci)
	{
		Call &c = calls[ci];
		c.rc = subq_ingest(env, sq[c.kind], c.host, NHOSTS, c.data.data(), c.data.size(), c.n, c.kind == SubQ::RESP ? nullptr : c.offs.data());
		return c.rc;
	}

	// (a) .. (d) over everything launched so far (the device is idle).  `all`: every call that returned GYS_OK must be there.
	void verify(bool all = true)
	{
		fake::sync();
		for (Call &c : calls) c.found = 0, c.sub = -1;
		for (SubQ::Kind kind : {SubQ::RESP, SubQ::CONN, SubQ::LSTATE}) {
			const SubQ &q = sq[kind];
			std::map<uint32_t, uint32_t> last_of_host, last_of_thread; // seq + 1 of the last call seen
			std::set<const uint8_t *> devs;
			for (size_t si = 0; si < log[kind].size(); ++si) {
				const Submission &s = *log[kind][si];
				devs.insert(s.dev);
				CHECK(s.fill > 0 && s.fill <= q.cap); // (d)
				auto take = [&](uint32_t id, uint64_t at, uint32_t host) -> Call * {
					if (!id || id > calls.size()) return nullptr;
					Call &c = calls[id - 1];
					CHECK(c.kind == kind && c.host == host);
					if (c.kind != kind) return nullptr;
					c.found++; // (a) exactly once
					c.sub = (int)si;
					const uint64_t b = kind == SubQ::RESP ? at * 24 : at;
					CHECK(b + c.data.size() <= s.bytes.size() && !memcmp(s.bytes.data() + b, c.data.data(), c.data.size())); // (a) byte-equal
					CHECK(c.seq + 1 > last_of_thread[c.thread]); // (b) (c) a thread's calls keep their order across submissions
					last_of_thread[c.thread] = c.seq + 1;
					return &c;
				};
				if (kind == SubQ::RESP) {
					CHECK(s.nrec == 0 && !s.segs.empty());
					std::set<uint32_t> hosts;
					for (size_t j = 0; j < s.segs.size(); ++j) {
						const uint64_t at = s.segs[j].first_event, end = j + 1 < s.segs.size() ? s.segs[j + 1].first_event : s.fill;
						CHECK(at < end && end <= s.fill && (j || at == 0));
						CHECK(hosts.insert(s.segs[j].host_slot).second); // (b) a host has at most one segment per submission
						if (at >= end || end > s.fill) continue;
						uint32_t id;
						memcpy(&id, s.bytes.data() + at * 24, 4);
						Call *c = take(id, at, s.segs[j].host_slot);
						CHECK(c && c->n == end - at);
						if (!c) continue;
						CHECK(c->seq + 1 > last_of_host[c->host]); // (b) a host's calls in call order
						last_of_host[c->host] = c->seq + 1;
					}
				} else {
					CHECK(s.nrec > 0 && s.nrec <= q.cap_recs && s.offs.size() == s.nrec); // (d)
					uint64_t next_at = 0;
					for (uint32_t r = 0; r < s.nrec;) {
						const uint64_t at = s.offs[r]; // (a call's first record is at its start)
						CHECK(at % 8 == 0 && at == next_at && at + 8 <= s.fill); // (c) 8-byte aligned, reservation order, nothing between the calls
						if (at + 8 > s.fill) break;
						uint32_t id;
						memcpy(&id, s.bytes.data() + at, 4);
						Call *c = take(id, at, id && id <= calls.size() ? calls[id - 1].host : 0);
						CHECK(c && r + c->n <= s.nrec);
						if (!c || r + c->n > s.nrec) break;
						bool rebased = true, named = true;
						for (uint32_t i = 0; i < c->n; ++i) {
							rebased = rebased && s.offs[r + i] == c->offs[i] + at; // (c) offsets rebased by the call's start
							named = named && (kind != SubQ::LSTATE || s.hosts[r + i] == c->host); // (c) the host-slot array names the caller's host
						}
						CHECK(rebased);
						CHECK(named);
						r += c->n;
						next_at = at + align_up(c->data.size(), 8);
					}
					CHECK(next_at == s.fill);
				}
			}
			CHECK((int)devs.size() <= q.nb); // (d) at most nb batches exist
		}
		for (const Call &c : calls) {
			CHECK(c.found <= 1);
			if (all && c.rc == GYS_OK) CHECK(c.found == 1);
		}
	}
};

static std::mt19937_64 g_rng;

// (a) (b) (c) (d) (g): 16 caller threads, every host owned by one thread, the three queues at once, seeded random call sizes (a few of many
// records or many bytes, so that batches fill up), a device that takes a little time over a submission (so that calls accumulate), and
// a 17th thread that flushes: every call that had returned before a flush began is on the stream when the flush returns
static void case_concurrent(int calls_per_thread)
{
	phase("16 threads", 120);
	Rig rig;
	rig.launch_us = 150;
	std::vector<std::vector<size_t>> mine(NTHREADS);
	for (uint32_t t = 0; t < NTHREADS; ++t)
		for (int s = 0; s < calls_per_thread; ++s) {
			const SubQ::Kind kind = (SubQ::Kind)(g_rng() % 3);
			const uint32_t host = t + NTHREADS * (uint32_t)(g_rng() % (NHOSTS / NTHREADS));
			const uint32_t roll = (uint32_t)(g_rng() % 100);
			uint32_t n = 1 + (uint32_t)(g_rng() % 300), words = ~0u;
			if (kind == SubQ::RESP) {
				if (roll < 3) n = (uint32_t)rig.sq[kind].cap; // a whole batch
				else if (roll < 10) n = 1500 + (uint32_t)(g_rng() % 1500);
			} else if (roll < 4) {
				n = rig.sq[kind].cap_recs / 2 - (uint32_t)(g_rng() % 3), words = 0; // as many records as a queued message may have
			} else if (roll < 8 && kind == SubQ::LSTATE) {
				n = 6000 + (uint32_t)(g_rng() % 2000), words = 48; // 1.2 .. 1.6 MiB of the batch's 4
			}
			mine[t].push_back(rig.add_call(g_rng, kind, host, t, (uint32_t)s, n, words));
		}
	std::atomic<uint32_t> returned[NTHREADS] = {};
	std::atomic<int> running{(int)NTHREADS};
	std::atomic<bool> go{false};
	std::vector<std::thread> th;
	for (uint32_t t = 0; t < NTHREADS; ++t)
		th.emplace_back([&, t] {
			while (!go.load()) std::this_thread::yield();
			for (size_t k = 0; k < mine[t].size(); ++k) {
				CHECK(rig.send(mine[t][k]) == GYS_OK);
				returned[t].store((uint32_t)k + 1, std::memory_order_release);
			}
			running--;
		});
	struct Flush {
		SubQ::Kind kind;
		uint32_t returned[NTHREADS];
		size_t launched;
	};
	std::vector<Flush> flushes;
	go = true;
	while (running.load()) {
		Flush f;
		f.kind = (SubQ::Kind)(flushes.size() % 3);
		for (uint32_t t = 0; t < NTHREADS; ++t) f.returned[t] = returned[t].load(std::memory_order_acquire);
		CHECK(subq_flush(rig.env, rig.sq[f.kind]) == GYS_OK);
		f.launched = rig.launched(f.kind);
		flushes.push_back(f);
		std::this_thread::sleep_for(std::chrono::microseconds(300));
	}
	for (auto &x : th) x.join();
	for (SubQ &q : rig.sq) CHECK(subq_flush(rig.env, q) == GYS_OK);
	rig.verify();
	for (const Flush &f : flushes) // (g)
		for (uint32_t t = 0; t < NTHREADS; ++t)
			for (uint32_t k = 0; k < f.returned[t]; ++k) {
				const Call &c = rig.calls[mine[t][k]];
				if (c.kind == f.kind) CHECK(c.sub >= 0 && (size_t)c.sub < f.launched);
			}
	uint64_t ncalls = 0, nsub = 0;
	for (SubQ &q : rig.sq) {
		std::lock_guard<std::mutex> g(q.mu);
		CHECK(q.calls >= q.submissions && q.submissions == rig.log[q.kind].size());
		ncalls += q.calls, nsub += q.submissions;
	}
	CHECK(ncalls == (uint64_t)NTHREADS * calls_per_thread);
	printf("16 threads: %llu calls in %llu submissions, %zu flushes\n", (unsigned long long)ncalls, (unsigned long long)nsub, flushes.size());
}

// (e) a lone caller with an idle device has its call submitted before the call returns
static void case_lone_caller()
{
	phase("lone caller", 30);
	Rig rig;
	for (SubQ::Kind kind : {SubQ::RESP, SubQ::CONN, SubQ::LSTATE})
		for (uint32_t k = 0; k < 12; ++k) { // (more calls than the queue has batches)
			CHECK(rig.send(rig.add_call(g_rng, kind, k % 3, 0, k, 1 + (uint32_t)(g_rng() % 50))) == GYS_OK);
			CHECK(rig.submissions(kind) == k + 1 && rig.launched(kind) == k + 1 && rig.pending(kind) == 0);
			fake::sync();
		}
	rig.verify();
	for (SubQ &q : rig.sq) {
		std::lock_guard<std::mutex> g(q.mu);
		CHECK(q.calls == 12 && q.tail_flushes == 0);
	}
}

// (f) with the device stalled and GYS_RQ_INFLIGHT submissions on it further calls return without submitting; after release the flusher
// submits the tail with no further call.  (d) too: a batch that has no room is sealed and leaves before the one opened after it.
static void case_tail(SubQ::Kind kind)
{
	phase("tail of a burst", 30);
	Rig rig;
	fake::pause();
	uint32_t k = 0;
	for (; k < GYS_RQ_INFLIGHT; ++k) CHECK(rig.send(rig.add_call(g_rng, kind, k, 0, k, 10)) == GYS_OK);
	CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT);
	for (; k < GYS_RQ_INFLIGHT + 3; ++k) CHECK(rig.send(rig.add_call(g_rng, kind, k, 0, k, 10)) == GYS_OK);
	CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT && rig.pending(kind) != 0);
	std::this_thread::sleep_for(std::chrono::milliseconds(5)); // (many of the flusher's 200 us: it must not submit while the device is busy)
	CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT);
	if (kind != SubQ::RESP) {
		// no room for this one (records: half a batch's, twice; bytes likewise): the open batch is sealed and leaves at once, stalled device or not
		const uint32_t half = rig.sq[kind].cap_recs / 2;
		CHECK(rig.send(rig.add_call(g_rng, kind, k, 0, k, half, 0)) == GYS_OK);
		++k;
		CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT);
		CHECK(rig.send(rig.add_call(g_rng, kind, k, 0, k, half, 0)) == GYS_OK);
		++k;
		CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT + 1);
	} else {
		CHECK(rig.send(rig.add_call(g_rng, kind, 2, 0, k, 10)) == GYS_OK); // host 2 has a segment in the open batch
		++k;
		CHECK(rig.submissions(kind) == GYS_RQ_INFLIGHT + 1);
	}
	const uint64_t before = rig.submissions(kind);
	CHECK(rig.pending(kind) != 0);
	fake::resume();
	CHECK(wait_for([&] { return rig.pending(kind) == 0 && rig.submissions(kind) == before + 1; }, 10000)); // no further call
	rig.verify();
	std::lock_guard<std::mutex> g(rig.sq[kind].mu);
	CHECK(rig.sq[kind].tail_flushes >= 1);
}

// (h) errors
static void case_errors(SubQ::Kind kind)
{
	phase("errors", 30);
	Rig rig;
	uint32_t k = 0;
	auto call = [&](uint32_t host) { return rig.send(rig.add_call(g_rng, kind, host, 0, k++, 20)); };
	// a failed launch of the batch that carries the caller's data: that caller gets the code
	rig.fail_launch_in = 1;
	g_err[0] = 0;
	CHECK(call(0) == GYS_ERR_HIP && strstr(g_err, "launch refused"));
	rig.calls.back().rc = -1; // (not delivered)
	CHECK(call(0) == GYS_OK);
	fake::sync();
	// a failure of a submission made for others (here: by the flusher) is parked and reported ONCE by the next call, whose data still arrives
	fake::pause();
	for (uint32_t h = 0; h < GYS_RQ_INFLIGHT + 1; ++h) CHECK(call(h) == GYS_OK);
	const size_t lost = rig.calls.size() - 1;
	const uint64_t before = rig.submissions(kind);
	rig.fail_launch_in = 1;
	fake::resume();
	CHECK(wait_for([&] { return rig.submissions(kind) == before + 1; }, 10000));
	fake::sync();
	rig.calls[lost].rc = -1;
	g_err[0] = 0;
	CHECK(call(5) == GYS_ERR_HIP && strstr(g_err, "launch refused"));
	rig.calls.back().rc = GYS_OK; // its data must be there all the same
	CHECK(rig.pending(kind) == 0 && call(6) == GYS_OK);
	fake::sync();
	// ... or by the next flush
	fake::pause();
	for (uint32_t h = 0; h < GYS_RQ_INFLIGHT + 1; ++h) CHECK(call(h) == GYS_OK);
	rig.calls.back().rc = -1;
	rig.fail_launch_in = 1;
	CHECK(subq_flush(rig.env, rig.sq[kind]) == GYS_ERR_HIP && strstr(g_err, "launch refused"));
	CHECK(subq_flush(rig.env, rig.sq[kind]) == GYS_OK);
	fake::resume();
	fake::sync();
	// an event in an error state is reaped: reported once, the free list does not drain, later callers do not block
	fake::fail_record_in = 2; // (`copied`, then `done` of the next submission)
	CHECK(call(0) == GYS_OK);
	fake::sync();
	g_err[0] = 0;
	CHECK(call(1) == GYS_ERR_HIP && strstr(g_err, kind == SubQ::RESP ? "response submission: launch failure" : "record submission: launch failure"));
	rig.calls.back().rc = GYS_OK;
	for (int i = 0; i < 3 * rig.sq[kind].nb; ++i) {
		CHECK(call(2) == GYS_OK);
		fake::sync();
	}
	{
		std::lock_guard<std::mutex> g(rig.sq[kind].mu);
		subq_reap(rig.sq[kind]);
		CHECK(rig.sq[kind].inflight.empty() && (int)rig.sq[kind].free.size() == rig.sq[kind].nb - (rig.sq[kind].open >= 0));
	}
	rig.verify();
}

// (i) a failed first-use allocation returns the error and the batch; the next caller completes it (both halves or none)
static void case_alloc_fails(SubQ::Kind kind)
{
	phase("allocation fails", 30);
	for (int half = 1; half <= 2; ++half) { // the pinned half, the device half
		Rig rig;
		const long blocks = fake::live_blocks;
		fake::fail_alloc_in = half;
		g_err[0] = 0;
		CHECK(rig.send(rig.add_call(g_rng, kind, 0, 0, 0, 5)) == GYS_ERR_HIP && strstr(g_err, "out of memory"));
		CHECK(fake::live_blocks == blocks);
		{
			std::lock_guard<std::mutex> g(rig.sq[kind].mu);
			CHECK((int)rig.sq[kind].free.size() == rig.sq[kind].nb && rig.sq[kind].open < 0);
		}
		for (uint32_t k = 1; k <= 8; ++k) {
			CHECK(rig.send(rig.add_call(g_rng, kind, 0, 0, k, 5)) == GYS_OK);
			fake::sync();
		}
		CHECK(fake::live_blocks == blocks + 2 * rig.sq[kind].nb);
		rig.verify();
	}
}

// (j) the ring
static void case_ring()
{
	phase("ring", 60);
	Rig rig;
	struct Seen {
		int slot;
		std::vector<uint8_t> bytes;
	};
	std::mutex mu;
	std::vector<std::unique_ptr<Seen>> seen;
	std::atomic<int> inside{0};
	bool track_slots = true; // (one caller at a time: nobody is growing a slot's buffers meanwhile)
	auto call = [&](uint32_t tag, uint64_t bytes, bool on_copy_stream) {
		return stage_call(
			rig.env, rig.ring, bytes, [&](uint8_t *pinned) { for (uint64_t i = 0; i < bytes; ++i) pinned[i] = (uint8_t)(tag + i); }, on_copy_stream, "ring call",
			[&](const uint8_t *dev) {
				CHECK(inside.fetch_add(1) == 0); // enq_mu is held
				auto s = std::make_unique<Seen>();
				Seen *sp = s.get();
				sp->slot = -1;
				for (int i = 0; i < NSTAGE && track_slots; ++i)
					if (rig.ring.slot[i].buf.dev == dev) sp->slot = i;
				inside.fetch_sub(1);
				fake::launch(rig.env.stream, [sp, dev, bytes] { sp->bytes.assign(dev, dev + bytes); });
				std::lock_guard<std::mutex> g(mu);
				seen.push_back(std::move(s));
				return GYS_OK;
			});
	};
	auto contents_ok = [&](size_t from, uint32_t tag0) {
		fake::sync();
		for (size_t i = from; i < seen.size(); ++i) {
			bool ok = !seen[i]->bytes.empty();
			for (size_t j = 0; j < seen[i]->bytes.size(); ++j) ok = ok && seen[i]->bytes[j] == (uint8_t)(tag0 + (i - from) + j);
			CHECK(ok);
		}
	};
	// slots are handed out oldest first; a burst shorter than the ring never waits, a stalled device or not
	fake::pause();
	for (uint32_t i = 0; i < NSTAGE - 4; ++i) CHECK(call(i, 100 + i, i & 1) == GYS_OK);
	CHECK(rig.ring.waits == 0);
	fake::resume();
	contents_ok(0, 0);
	for (uint32_t i = NSTAGE - 4; i < 2 * NSTAGE + 3; ++i) {
		CHECK(call(i, 100 + i, i & 1) == GYS_OK);
		fake::sync();
	}
	for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i]->slot == (int)(i % NSTAGE));
	track_slots = false;
	CHECK(rig.ring.waits == 0);
	contents_ok(0, 0);
	// a wrapped ring with the device stalled counts one wait, and waits
	const size_t n0 = seen.size();
	fake::pause();
	for (uint32_t i = 0; i < NSTAGE; ++i) CHECK(call(50 + i, 64, true) == GYS_OK);
	CHECK(rig.ring.waits == 0);
	std::atomic<bool> back{false};
	std::thread late([&] {
		CHECK(call(50 + NSTAGE, 64, true) == GYS_OK);
		back = true;
	});
	CHECK(wait_for([&] { return rig.ring.waits == 1; }, 10000));
	std::this_thread::sleep_for(std::chrono::milliseconds(2));
	CHECK(!back);
	fake::resume();
	late.join();
	CHECK(rig.ring.waits == 1);
	contents_ok(n0, 50);
	// a failed grow returns the slot (and a runtime error text begins with the caller's prefix -- none here: the allocator's own)
	const size_t n1 = seen.size();
	fake::fail_alloc_in = 1;
	CHECK(call(0, 4u << 20, false) == GYS_ERR_HIP && strstr(g_err, "out of memory"));
	{
		std::lock_guard<std::mutex> g(rig.ring.mu);
		CHECK(rig.ring.free.size() == (size_t)NSTAGE);
	}
	CHECK(seen.size() == n1);
	// 16 threads: every call's bytes arrive, whichever stream copies
	std::vector<std::thread> th;
	std::atomic<int> bad{0};
	for (uint32_t t = 0; t < NTHREADS; ++t)
		th.emplace_back([&, t] {
			for (uint32_t k = 0; k < 12; ++k) bad += call(t * 16 + k, 2000 + 37 * t + k, (t + k) & 1) != GYS_OK;
		});
	for (auto &x : th) x.join();
	fake::sync();
	CHECK(bad == 0 && seen.size() == n1 + NTHREADS * 12);
	for (size_t i = n1; i < seen.size(); ++i) {
		const std::vector<uint8_t> &b = seen[i]->bytes;
		bool ok = b.size() >= 2000;
		for (size_t j = 1; j < b.size(); ++j) ok = ok && b[j] == (uint8_t)(b[0] + j);
		CHECK(ok);
	}
	std::lock_guard<std::mutex> g(rig.ring.mu);
	CHECK(rig.ring.free.size() == (size_t)NSTAGE);
}

// (k) teardown: with data in the open batch and the flusher waiting for the device; with the flusher asleep on an empty queue; with a queue
// that was never used.  It joins, and nothing is left: events and blocks are counted here, LeakSanitizer and AddressSanitizer see the rest.
static void case_teardown()
{
	phase("teardown", 30);
	const long blocks = fake::live_blocks, events = fake::live_events;
	{
		Rig rig;
		fake::pause();
		for (uint32_t k = 0; k < GYS_RQ_INFLIGHT + 2; ++k) CHECK(rig.send(rig.add_call(g_rng, SubQ::CONN, k, 0, k, 30)) == GYS_OK);
		CHECK(rig.pending(SubQ::CONN) != 0);
		CHECK(rig.send(rig.add_call(g_rng, SubQ::RESP, 0, 0, 9, 30)) == GYS_OK); // submitted: its flusher sleeps
		int si;
		CHECK(stage_acquire(rig.env, rig.ring, 100, &si) == GYS_OK);
		stage_release(rig.ring, si);
		CHECK(fake::live_events > events && fake::live_blocks > blocks);
		fake::resume();
	}
	CHECK(fake::live_blocks == blocks && fake::live_events == events && fake::bad_frees == 0);
	{
		Rig idle;
	}
	CHECK(fake::live_blocks == blocks && fake::live_events == events);
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	const int calls_per_thread = argc > 2 ? atoi(argv[2]) : 60;
	g_rng.seed(seed * 0x9E3779B97F4A7C15ull + 1);
	std::thread dev(fake::device_thread), dog(watchdog);
	case_lone_caller();
	for (SubQ::Kind kind : {SubQ::RESP, SubQ::CONN, SubQ::LSTATE}) {
		case_tail(kind);
		case_errors(kind);
		case_alloc_fails(kind);
	}
	case_ring();
	case_teardown();
	case_concurrent(calls_per_thread);
	g_deadline_ms = -1;
	{
		std::lock_guard<std::mutex> g(fake::m);
		fake::quit = true;
		fake::cv.notify_all();
	}
	dev.join();
	dog.join();
	CHECK(fake::live_blocks == 0 && fake::live_events == 0 && fake::bad_frees == 0);
	if (g_fail) {
		printf("%d checks failed\n", g_fail.load());
		return 1;
	}
	printf("subq ok\n");
	return 0;
}
