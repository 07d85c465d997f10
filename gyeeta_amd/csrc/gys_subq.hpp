// gys_subq.hpp -- the host-pointer ingest boundary (gys_ingest_resp_events / _tcp_conn / _listener_state and their siblings):
// the submission queues ("group commit") and the ring of pinned staging slots.  The library's only multi-threaded code.  Host code: the
// HIP runtime calls, gys_devmem.hpp and gys_resp_seg of gysketch.h; no gys_ctx, no kernel.  What it uses of the context is bound once at
// gys_create (IngestEnv): the device, the two streams, enq_mu, and ONE callable that launches a copied batch.
// tests/cpp/test_subq.cc runs it on the CPU over a fake runtime with a device thread, under ThreadSanitizer and AddressSanitizer.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gys_devmem.hpp"

namespace gys {

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

constexpr uint64_t GYS_RQ_EVENTS = 1u << 21; // events per combined batch (48 MiB pinned + 48 MiB device each)
constexpr uint64_t GYS_CQ_CONN_BYTES = 16u << 20, GYS_CQ_LSTATE_BYTES = 4u << 20; // record bytes per combined batch
constexpr size_t GYS_RQ_INFLIGHT = 2; // submissions executing / queued on the GPU before new calls start to accumulate

// Submission queues of the host-pointer calls ("group commit", SURVEY 8b second option): one for gys_ingest_resp_events, one for
// gys_ingest_tcp_conn (TCP_CONN_NOTIFY), one for gys_ingest_listener_state (LISTENER_STATE_NOTIFY).  The calls of all L2 threads are
// appended to ONE pinned batch and a batch is copied and launched once, so that the fixed cost of a submission is paid per batch
// instead of per call: the ~12 launches of a response batch per 65536-event call; for the records, through the 16-slot staging ring,
// an H2D copy, two event records, a stream wait and a launch -- five runtime calls of ~5 us each under enq_mu for a 2048-record
// (0.57 MB) or 512-record (45 KB) message: 69 M connection records/s and 24 M listener records/s from 16 threads, a third and a
// twentieth of what the link carries, with the ring wrapping all the time (gys_counters.stage_waits).
// The protocol (subq_* below): a caller reserves its place in the open batch under mu, copies outside any lock (`writers` counts the
// copies in progress), and whoever finds no submission being made submits what has accumulated.  A lone caller submits its own call at
// once: no added latency.  While GYS_RQ_INFLIGHT submissions are still executing on the GPU, further calls accumulate and go out
// together as soon as one of them has finished -- the GPU always has the next submission queued behind the running one, and the fixed
// cost is amortised exactly when the GPU is the bottleneck.  Batches are submitted in the order they were sealed.  The tail of a
// burst: calls that found GYS_RQ_INFLIGHT submissions on the GPU left their data in the open batch, and after the burst nobody calls
// again -- a flusher thread (started with the first queued call) submits that batch once a submission has retired.
// Responses: a segment per call, and a host appears at most once per batch (its keys see their per-call value multisets in call
// order: the digests stay bit-identical to per-call ingestion).  Records: the records, then an offset (and, for listener states, the
// sender's host slot) per record; they keep the order in which the calls reserved their place, so "the last record of a listener
// wins" holds across the messages of a batch as it does across calls.
struct SubQ {
	enum Kind { RESP, CONN, LSTATE } kind = RESP; // (also its index in gys_ctx::sq)
	struct Batch {
		PinnedPair<uint8_t> buf;            // RESP: events; else [records: cap][offset per record: u32 x cap_recs][host slot per record: u32 x cap_recs]
		uint64_t fill = 0;                  // RESP: events; else record bytes (8-byte aligned per call)
		uint32_t nrec = 0;                  // records (not RESP)
		std::vector<gys_resp_seg> segs;     // RESP: a segment per call
		hipEvent_t done = nullptr;          // behind the batch's kernels: its buffers are not reused before
		hipEvent_t copied = nullptr;        // the batch's H2D copies on the copy stream (the engine stream waits for it before the batch's kernels)
		uint32_t writers = 0;
	} b[6];
	int nb = 0;                     // batches in use: 6 (RESP) / 4
	uint64_t cap = 0, buf_bytes = 0; // per batch: `fill` it holds, size of buf
	uint32_t cap_recs = 0;
	std::mutex mu;
	std::condition_variable cv;
	std::deque<int> free, sealed, inflight; // sealed: awaiting submission, oldest first; inflight: submitted, GPU not done yet
	int open = -1;
	bool submitting = false;
	int async_rc = 0; // first error of a submission made on behalf of other callers; surfaces at the next call
	std::string async_err;
	uint64_t calls = 0, submissions = 0, tail_flushes = 0;
	std::vector<uint32_t> host_stamp; // RESP: host -> stamp of the open batch it is in
	uint32_t stamp = 0;
	std::condition_variable fcv;
	std::thread flusher;
	bool flusher_on = false, stop = false;
	const char *word() const { return kind == RESP ? "response" : "record"; } // (error texts)
};

// What the queues and the ring use of the context.  `launch` enqueues the kernels of a copied batch on `stream`: the batch starts at `dev`;
// RESP: `fill` events in `segs`; else `nrec` records, their offsets at dev + q.cap and (LSTATE) their host slots behind those.  It is
// called with *enq_mu held.
struct IngestEnv {
	int device = 0;
	hipStream_t stream = nullptr, copy_stream = nullptr;
	std::mutex *enq_mu = nullptr; // the enqueue: stream order, the engine's shared flags
	uint64_t max_batch_events = 0;
	std::function<int(SubQ::Kind, const uint8_t *, uint64_t, uint32_t, const std::vector<gys_resp_seg> &)> launch; // (kind, dev, fill, nrec, segs)
};

inline void subq_init(const IngestEnv &env, SubQ &q, SubQ::Kind kind)
{
	q.kind = kind;
	if (kind == SubQ::RESP) {
		q.nb = 6;
		q.cap = std::min<uint64_t>(GYS_RQ_EVENTS, std::max<uint64_t>(env.max_batch_events, 1));
		q.buf_bytes = q.cap * 24;
	} else {
		q.nb = 4;
		q.cap = kind == SubQ::CONN ? GYS_CQ_CONN_BYTES : GYS_CQ_LSTATE_BYTES;
		q.cap_recs = (uint32_t)(q.cap / (kind == SubQ::CONN ? 280u : 88u));
		q.buf_bytes = q.cap + (uint64_t)q.cap_recs * 8;
	}
	for (int i = 0; i < q.nb; ++i) q.free.push_back(i);
}

// submits batch b of q (sealed, no writers); q.mu NOT held
inline int subq_submit_one(const IngestEnv &env, SubQ &q, SubQ::Batch &b)
{
	const bool resp = q.kind == SubQ::RESP;
	int rc = GYS_OK;
	std::lock_guard<std::mutex> g(*env.enq_mu);
	// copy on its own stream, kernels on the engine stream behind an event: with everything on one stream the 48-MiB copy of a response
	// submission (0.85 ms at 57 GB/s) and its kernels alternate; the batch's buffers are not reused before `done` has fired
	hipStream_t cs = env.copy_stream;
	const uint64_t off_at = q.cap, host_at = q.cap + (uint64_t)q.cap_recs * 4;
	hipError_t e = hipMemcpyAsync(b.buf.dev, b.buf.host, resp ? b.fill * 24 : b.fill, hipMemcpyHostToDevice, cs);
	if (e == hipSuccess && !resp) e = hipMemcpyAsync(b.buf.dev + off_at, b.buf.host + off_at, (uint64_t)b.nrec * 4, hipMemcpyHostToDevice, cs);
	if (e == hipSuccess && q.kind == SubQ::LSTATE) e = hipMemcpyAsync(b.buf.dev + host_at, b.buf.host + host_at, (uint64_t)b.nrec * 4, hipMemcpyHostToDevice, cs);
	if (e == hipSuccess) e = hipEventRecord(b.copied, cs);
	if (e == hipSuccess) e = hipStreamWaitEvent(env.stream, b.copied, 0);
	if (e == hipSuccess) {
		rc = env.launch(q.kind, b.buf.dev, b.fill, b.nrec, b.segs);
		e = hipEventRecord(b.done, env.stream);
	}
	if (e != hipSuccess) {
		set_err("%s submission: %s", q.word(), hipGetErrorString(e));
		rc = GYS_ERR_HIP;
	}
	return rc;
}

// q.mu held: batches whose kernels have finished go back to the free list
inline void subq_reap(SubQ &q)
{
	// anything but "not ready" ends a submission's stay on the in-flight list: an event in an error state never turns into hipSuccess, and
	// a head that is never reaped would leave every later caller waiting once the free list has drained
	while (!q.inflight.empty()) {
		const hipError_t e = hipEventQuery(q.b[q.inflight.front()].done);
		if (e == hipErrorNotReady) break;
		if (e != hipSuccess && !q.async_rc) {
			q.async_rc = GYS_ERR_HIP;
			q.async_err = std::string(q.word()) + " submission: " + hipGetErrorString(e);
		}
		q.free.push_back(q.inflight.front());
		q.inflight.pop_front();
	}
	(void)hipGetLastError(); // (hipErrorNotReady is not an error)
}

// With q.mu held (lk): submit, oldest first, every sealed batch whose writers are done -- and the open batch too when `all`, or when it
// has data, no writer, and fewer than GYS_RQ_INFLIGHT submissions are still on the GPU.  Returns the first error of a batch that
// carried the caller's own data (`mine`), other errors are parked in q.async_rc.
inline int subq_drain(const IngestEnv &env, SubQ &q, std::unique_lock<std::mutex> &lk, int mine, bool all)
{
	int my_rc = GYS_OK;
	for (;;) {
		if (q.submitting) { // (first time round, or after the wait for a batch's writers below)
			if (!all) return my_rc; // the thread inside the submission picks up what accumulates
			q.cv.wait(lk, [&] { return !q.submitting; });
		}
		if (q.sealed.empty() && q.open >= 0 && q.b[q.open].fill && (all || q.b[q.open].writers == 0)) { // (all: its writers are waited for below)
			subq_reap(q);
			if (all || q.inflight.size() < GYS_RQ_INFLIGHT) {
				q.sealed.push_back(q.open);
				q.open = -1;
			}
		}
		if (q.sealed.empty()) break;
		const int bi = q.sealed.front();
		SubQ::Batch &b = q.b[bi];
		if (b.writers) {
			if (!all) break; // its last writer drains
			q.cv.wait(lk, [&] { return b.writers == 0; });
			continue; // the lock was released: the batch's last writer may have taken it from the list, and may be submitting it
		}
		q.sealed.pop_front();
		q.submitting = true;
		lk.unlock();
		const int rc = subq_submit_one(env, q, b);
		lk.lock();
		q.submitting = false;
		q.submissions++;
		b.fill = 0;
		b.nrec = 0;
		b.segs.clear();
		q.inflight.push_back(bi);
		q.cv.notify_all();
		if (rc) {
			if (bi == mine) my_rc = rc;
			else if (!q.async_rc) {
				q.async_rc = rc;
				q.async_err = g_err;
			}
		}
	}
	return my_rc;
}

// q.mu held: the error of a submission made for other callers (or by the flusher) is reported once, by the first call that comes by
inline int subq_parked_error(SubQ &q)
{
	const int rc = q.async_rc;
	if (rc) {
		set_err("%s", q.async_err.c_str());
		q.async_rc = 0;
	}
	return rc;
}

// everything the queue holds is on the stream when this returns (entry points other than the concurrent ingest calls start with it)
inline int subq_flush(const IngestEnv &env, SubQ &q)
{
	std::unique_lock<std::mutex> lk(q.mu);
	if (q.open >= 0 || !q.sealed.empty() || q.submitting) (void)subq_drain(env, q, lk, -1, true); // (no batch of this caller's: errors are parked)
	return subq_parked_error(q);
}

// flusher thread of a submission queue: sleeps until a call leaves data behind in the open batch, then tries every 200 us to submit
// it (subq_drain submits only while fewer than GYS_RQ_INFLIGHT submissions are on the GPU); an error lands in q.async_rc for the next caller
inline void subq_flusher(const IngestEnv *envp, SubQ *qp)
{
	const IngestEnv &env = *envp;
	SubQ &q = *qp;
	(void)hipSetDevice(env.device);
	std::unique_lock<std::mutex> lk(q.mu);
	for (;;) {
		q.fcv.wait(lk, [&] { return q.stop || (q.open >= 0 && q.b[q.open].fill != 0); });
		if (q.stop) break;
		// the GPU is the bottleneck while GYS_RQ_INFLIGHT submissions are on it: wait for the oldest one's event (outside the lock) rather than
		// wake every 200 us to find nothing to do; otherwise give the burst 200 us to bring more calls before its tail goes out
		hipEvent_t busy = q.inflight.size() >= GYS_RQ_INFLIGHT ? q.b[q.inflight.front()].done : nullptr;
		lk.unlock();
		if (busy) (void)hipEventSynchronize(busy);
		else std::this_thread::sleep_for(std::chrono::microseconds(200));
		lk.lock();
		if (q.stop) break;
		if (q.open >= 0 && q.b[q.open].fill && q.b[q.open].writers == 0 && !q.submitting) {
			const uint64_t before = q.submissions;
			(void)subq_drain(env, q, lk, -1, false);
			if (q.submissions != before) q.tail_flushes++;
		}
	}
}

// one call of the sender in slot `host` of `nhosts` registered hosts.  Responses: n events of 24 bytes at `data` (offs unused).
// Records: one message, `bytes` of records at `data`, offs[i] = offset of record i of n in it.
inline int subq_ingest(const IngestEnv &env, SubQ &q, uint32_t host, size_t nhosts, const void *data, uint64_t bytes, uint32_t n, const uint32_t *offs)
{
	const bool resp = q.kind == SubQ::RESP;
	const uint64_t need = resp ? n : align_up(bytes, 8); // of a batch's `fill`
	std::unique_lock<std::mutex> lk(q.mu);
	if (!q.flusher_on) {
		q.flusher_on = true;
		q.flusher = std::thread(subq_flusher, &env, &q);
	}
	// (an earlier submission made for other callers may have failed: that error is reported once, by the first call that comes by -- AFTER
	// the caller's own data has been queued below, never instead of it)
	q.calls++;
	if (resp && q.host_stamp.size() < nhosts) q.host_stamp.resize(nhosts, 0);
	int bi;
	for (;;) {
		if (q.open < 0) {
			subq_reap(q);
			if (q.free.empty()) {
				if (!q.inflight.empty()) { // every batch is on the GPU: wait for the oldest (outside the lock), then look again
					hipEvent_t ev = q.b[q.inflight.front()].done;
					lk.unlock();
					(void)hipEventSynchronize(ev);
					lk.lock();
				} else {
					q.cv.wait(lk, [&] { return !q.free.empty() || !q.inflight.empty(); }); // (sealed / being submitted by others)
				}
				continue;
			}
			bi = q.free.front();
			q.free.pop_front();
			SubQ::Batch &nb = q.b[bi];
			lk.unlock(); // (first-use allocation: outside the lock; the batch is not visible yet)
			// the buffers (both or none: PinnedPair) and the two events; what a failure leaves built, the next caller of this batch completes
			int arc = nb.buf.cap ? GYS_OK : nb.buf.grow(q.buf_bytes, 0);
			hipError_t e = hipSuccess;
			if (!arc && !nb.done) e = hipEventCreateWithFlags(&nb.done, hipEventDisableTiming);
			if (!arc && e == hipSuccess && !nb.copied) e = hipEventCreateWithFlags(&nb.copied, hipEventDisableTiming);
			if (e != hipSuccess) {
				set_err("%s batch events: %s", q.word(), hipGetErrorString(e));
				arc = GYS_ERR_HIP;
			}
			lk.lock();
			if (arc) {
				q.free.push_back(bi);
				q.cv.notify_all();
				return arc;
			}
			if (q.open >= 0) { // another caller opened one meanwhile
				q.free.push_front(bi);
				q.cv.notify_all();
				continue;
			}
			q.open = bi;
			++q.stamp;
		}
		bi = q.open;
		const SubQ::Batch &ob = q.b[bi];
		if (ob.fill + need <= q.cap && (resp ? q.host_stamp[host] != q.stamp : ob.nrec + n <= q.cap_recs)) break;
		// no room, or the host already has a segment in this batch: seal it (submitted before anything opened later)
		q.sealed.push_back(bi);
		q.open = -1;
		(void)subq_drain(env, q, lk, -1, false); // (no batch of this caller's yet: errors are parked, the result is always GYS_OK)
	}
	SubQ::Batch &b = q.b[bi];
	const uint64_t at = b.fill;
	const uint32_t r0 = b.nrec;
	b.fill += need;
	if (resp) {
		b.segs.push_back(gys_resp_seg{host, 0, at});
		q.host_stamp[host] = q.stamp;
	} else {
		b.nrec += n;
	}
	b.writers++;
	lk.unlock();
	if (resp) {
		memcpy(b.buf.host + at * 24, data, (uint64_t)n * 24);
	} else {
		memcpy(b.buf.host + at, data, bytes);
		uint32_t *o = (uint32_t *)(b.buf.host + q.cap) + r0;
		for (uint32_t i = 0; i < n; ++i) o[i] = offs[i] + (uint32_t)at;
		if (q.kind == SubQ::LSTATE) std::fill_n(o + q.cap_recs, n, host);
	} // the caller's buffer is free from here on
	lk.lock();
	b.writers--;
	if (b.writers == 0) q.cv.notify_all();
	int rc = subq_drain(env, q, lk, bi, false);
	if (q.open >= 0 && q.b[q.open].fill) q.fcv.notify_one(); // data stays behind in the open batch: the flusher sees to it if no call follows
	if (!rc) rc = subq_parked_error(q);
	return rc;
}

// ---- the staging ring.  A call that does not go through a queue (a message of many messages' size, an IPv6 response call,
// gys_ingest_active_conns) copies the caller's records into a slot's pinned buffer (the caller's buffer is free when the call returns --
// the reference's pone points into the L1 receive buffer, valid only for the call), enqueues ONE H2D copy + the kernels and returns
// without waiting for the GPU; a slot is reused after the event recorded behind its kernels has fired.  Up to MAX_L2_MISC_THREADS = 16
// L2 threads (server/gy_mconnhdlr.h:60) call concurrently: slots are handed out under mu, the memcpy into pinned memory runs outside
// any lock, the enqueue under enq_mu.
struct Stage {
	PinnedPair<uint8_t> buf;
	hipEvent_t done = nullptr;
	hipEvent_t copied = nullptr; // (record batches: the slot's H2D copy on the copy stream)
};
constexpr int NSTAGE = 16;

struct StageRing {
	Stage slot[NSTAGE];
	std::deque<int> free; // handed out OLDEST FIRST (pop_front / push_back): a slot's event has normally fired long before the slot comes round again
	std::mutex mu;
	std::condition_variable cv;
	std::atomic<uint64_t> waits{0}; // times a host-pointer call found its ring slot still in flight and waited for the GPU
	StageRing()
	{
		for (int i = 0; i < NSTAGE; ++i) free.push_back(i);
	}
};

inline void stage_release(StageRing &r, int idx)
{
	std::lock_guard<std::mutex> lk(r.mu);
	r.free.push_back(idx);
	r.cv.notify_one();
}

inline int stage_acquire(const IngestEnv &env, StageRing &r, uint64_t bytes, int *idx)
{
	int i;
	{
		std::unique_lock<std::mutex> lk(r.mu);
		r.cv.wait(lk, [&] { return !r.free.empty(); });
		i = r.free.front();
		r.free.pop_front();
	}
	Stage &st = r.slot[i];
	// the calling (L2) thread's current device is whatever it used last -- 0 for a fresh thread: the slot's buffers, the copy and the
	// kernels must live on the context's device
	hipError_t e = hipSetDevice(env.device);
	if (e == hipSuccess && !st.done) e = hipEventCreateWithFlags(&st.done, hipEventDisableTiming);
	if (e == hipSuccess && !st.copied) e = hipEventCreateWithFlags(&st.copied, hipEventDisableTiming);
	if (e == hipSuccess && hipEventQuery(st.done) == hipErrorNotReady) r.waits++;
	(void)hipGetLastError();
	if (e == hipSuccess) e = hipEventSynchronize(st.done); // the kernels that read this slot last time are done (no-op unless the ring wrapped)
	int rc = GYS_OK;
	if (e != hipSuccess) {
		set_err("staging slot: %s", hipGetErrorString(e));
		rc = GYS_ERR_HIP;
	} else if (bytes > st.buf.cap) {
		rc = st.buf.grow(align_up(bytes, 4096), 1u << 20);
	}
	if (rc) {
		stage_release(r, i);
		return rc;
	}
	*idx = i;
	return GYS_OK;
}

// One call through a ring slot: fill(pinned buffer) writes `bytes` (outside any lock); then, under enq_mu, ONE H2D copy -- on the copy
// stream with the engine stream waiting for the slot's `copied` event (as for the queues' submissions: the copy of one message runs
// under the kernels of the message before it), or on the engine stream itself --, launch(device buffer) and the `done` record; no wait
// for the GPU.  The slot goes back on every path.  `what` begins the text of a runtime error.
template <class Fill, class Launch>
int stage_call(const IngestEnv &env, StageRing &r, uint64_t bytes, Fill fill, bool on_copy_stream, const char *what, Launch launch)
{
	int si;
	int rc = stage_acquire(env, r, bytes, &si);
	if (rc) return rc;
	Stage &st = r.slot[si];
	fill(st.buf.host); // the caller's buffer is free from here on
	{
		std::lock_guard<std::mutex> g(*env.enq_mu);
		hipError_t e = hipMemcpyAsync(st.buf.dev, st.buf.host, bytes, hipMemcpyHostToDevice, on_copy_stream ? env.copy_stream : env.stream);
		if (e == hipSuccess && on_copy_stream) e = hipEventRecord(st.copied, env.copy_stream);
		if (e == hipSuccess && on_copy_stream) e = hipStreamWaitEvent(env.stream, st.copied, 0);
		if (e == hipSuccess) {
			rc = launch(st.buf.dev);
			e = hipEventRecord(st.done, env.stream);
		}
		if (e != hipSuccess) {
			set_err("%s: %s", what, hipGetErrorString(e));
			rc = GYS_ERR_HIP;
		}
	}
	stage_release(r, si);
	return rc;
}

// ---- teardown (no call is in progress or follows).  The flushers are stopped and joined (what an open batch still holds goes with the
// context); then sync_stream() -- the engine waits for its stream, behind which nothing reads a batch or a slot any more --; then the
// batches' and the slots' events are destroyed.  The buffers go with their owners.
template <class Sync>
void ingest_teardown(SubQ *sq, int nq, StageRing &r, Sync sync_stream)
{
	for (int i = 0; i < nq; ++i) {
		SubQ &q = sq[i];
		if (!q.flusher_on) continue;
		{
			std::lock_guard<std::mutex> g(q.mu);
			q.stop = true;
		}
		q.fcv.notify_all();
		if (q.flusher.joinable()) q.flusher.join();
		q.flusher_on = false;
	}
	sync_stream();
	for (int i = 0; i < nq; ++i)
		for (auto &b : sq[i].b) {
			if (b.done) hipEventDestroy(b.done);
			if (b.copied) hipEventDestroy(b.copied);
			b.done = b.copied = nullptr;
		}
	for (auto &st : r.slot) {
		if (st.done) hipEventDestroy(st.done);
		if (st.copied) hipEventDestroy(st.copied);
		st.done = st.copied = nullptr;
	}
}

} // namespace gys
