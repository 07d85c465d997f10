/*
 * gysketch.h -- C ABI of libgysketch.so, the MI355X-native streaming-sketch aggregation engine that replaces the inside of
 * Gyeeta's madhava/shyama roll-up path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Each entry point names the reference interface it replaces (file:line under the Gyeeta source tree).  The reference has no
 * FFI layer: its boundary is a set of C++ member functions called from the L2 dispatch switch
 * (server/gy_mconnhdlr.cc:4700-4792); gyeeta_amd/csrc/gys_mconn_shim.hpp gives those same C++ signatures on top of this ABI
 * and INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - All functions return 0 (GYS_OK) or a negative GYS_ERR_* code; nothing throws across the boundary
 *     (reference: bool return + GY_CATCH_EXCEPTION, gy_mconnhdlr.cc:4771-4774).
 *   - "batch"/"pend" pairs follow the reference iteration convention
 *     for (i < n && (uint8_t*)p < pendptr; p += p->get_elem_size())   (gy_mconnhdlr.cc:9130, :11175).
 *     Host buffers are only read during the call (the reference's DB_WRITE_ARR owns them, gy_mconnhdlr.h:350-442).
 *   - *_dev variants take DEVICE pointers to batches already resident in HBM (the measured configuration).
 *   - A context is bound to one GPU and one HIP stream; calls on one context must be serialised by the caller
 *     (one context per L2 thread pool, or an external mutex; the reference serialises per host with connlistenmutex_).
 */
#ifndef GYSKETCH_H
#define GYSKETCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GYS_ABI_VERSION 7

enum {
	GYS_OK = 0,
	GYS_ERR_INVAL = -1,     /* bad argument / malformed batch */
	GYS_ERR_NOMEM = -2,     /* capacity (hosts, services, batch staging) exhausted */
	GYS_ERR_HIP = -3,       /* HIP runtime error (gys_last_error() has the text) */
	GYS_ERR_NOTFOUND = -4,  /* unknown host / service */
	GYS_ERR_NOT_OWNER = -5, /* host is sharded to another rank (jhash2(machine_id) % nranks != rank) */
	GYS_ERR_STATE = -6,     /* call sequence error (e.g. window_finish without window_prepare) */
	GYS_ERR_INTERNAL = -7   /* a C++ exception other than an allocation failure inside the library (never crosses the boundary) */
};

/* bucket-hash kinds == the reference's hash classes, common/gy_statistics.h:1565-2063 */
enum {
	GYS_RESP_TIME_HASH = 0,   /* :1674 */
	GYS_SEMI_LOG_HASH = 1,    /* :1729 */
	GYS_SEMI_LOG_HASH_LO = 2, /* :1782 */
	GYS_DURATION_HASH = 3,    /* :1835 */
	GYS_HASH_10_5000 = 4,     /* :1908 */
	GYS_HASH_5_250 = 5,       /* :1960 */
	GYS_HASH_1_3000 = 6,      /* :2013 */
	GYS_PERCENT_HASH = 7,     /* :1624 */
	GYS_NUM_HASH_KINDS = 8
};

#define GYS_MAX_BUCKETS 16 /* all reference hash classes have <= 15 buckets; records are padded to 16 slots */
#define GYS_TD_NB 200      /* t-digest clusters per key (2 x the delta = 100 the reference hands to Postgres tdigest, common/gy_query_common.cc:1855) */
#define GYS_TD_PEND_CAP 896 /* values a key's t-digest buffers before it is re-clustered, by default (== GYS_TDIGEST_PEND_CAP); gys_config.td_pend_cap */
#define GYS_TD_PEND_CAP_MAX 3968 /* + 128 = 4096: the largest merge the one-workgroup value-bin kernel takes */
#define GYS_HLL_P 14       /* global distinct-flow HLL precision: 16384 u8 registers */
#define GYS_CMS_D 4
#define GYS_CMS_W 65536
#define GYS_NSTATES 6      /* OBJ_STATE_E STATE_IDLE..STATE_DOWN, common/gy_json_field_maps.h:242-250 */
#define GYS_TOPN 10        /* per-host top-N, server/gy_mconnhdlr.h:961 */

typedef struct gys_ctx gys_ctx;

typedef struct {
	uint32_t struct_size;      /* = sizeof(gys_config) */
	int32_t device;            /* HIP device ordinal, -1 = current device */
	uint32_t rank, nranks;     /* shard of the host-id space owned by this context; 0,1 for single GPU */
	uint32_t max_hosts;        /* partha capacity (reference: MAX_PARTHA_PER_MADHAVA = 512 per madhava) */
	uint32_t max_services;     /* listener capacity across all hosts */
	uint32_t max_clusters;     /* cluster-name capacity (MS_CLUSTER_STATE::MAX_NUM_CLUSTERS = 512) */
	uint32_t enable_tdigest;   /* per-service t-digest of response times */
	uint32_t svc_hll_p;        /* per-service distinct-client HLL precision (0 = off, 4..10) */
	uint32_t resp_path;        /* 0 = choose per batch; 1 = always the general (global table + atomics) pipeline; 2 = prefer the
	                              host-local pipeline (LDS sub-table per host segment) whenever the batch qualifies; 3 = as 2, and
	                              segments longer than 65536 events are cut into parts (split form: few hosts, long segments) */
	uint64_t max_batch_events; /* largest resp-event batch one ingest call may carry (t-digest staging capacity) */
	void *stream;              /* hipStream_t to run on; NULL = the context creates its own */
	void *reduce_arena;        /* optional caller-owned DEVICE buffer for the all-reducible registers (e.g. a torch tensor so */
	uint64_t reduce_arena_bytes; /* that torch.distributed/RCCL can reduce it in place); NULL = the context allocates it  */
	uint32_t enable_levels;    /* multi-level windows + per-service QPS / active-connection histograms (see "multi-level windows" below):
	                              1 = all four levels (5 s / 300 s / 5 days / all; 21 hist records = 5.4 KB of HBM per service; every window
	                                  close brings the records of every service touched in the window up to date -- what the reference's 5-s
	                                  flush does per listener);
	                              2 = without the 5-s level (300 s / 5 days / all): a close touches the services only when it crosses a ring
	                                  boundary (every 30 s); level 0 and gys_scan_listener_state_dev answer GYS_ERR_STATE, a period that
	                                  folly would answer from the 5-s ring is answered from the 300-s ring */
	uint32_t td_buf_values;    /* entries of a service's value buffer (td_pend_cap + 64 .. 16384; 0 = sized to max_services): the values
	                              waiting for the next t-digest merge plus room for one batch's values of the service */
	uint32_t conn_pair_cms;    /* TCP_CONN_NOTIFY records also feed a Count-Min pair OF THEIR OWN keyed by (ser_glob_id_, cli_task_aggr_id_): connections
	                              (u32 table) and bytes (u64 table) per (listener, client task group) -- the roll-up MCONN_HANDLER keeps in
	                              connlistenmap_ / connclientmap_ (server/gy_msocket.h:240-290, filled by add_tcp_conn_cli / _ser,
	                              server/gy_mconnhdlr.cc:8643-9050).  8 more device atomics per record; off by default */
	uint32_t td_pend_cap;      /* values a service's t-digest buffers before it is re-clustered: 0 = GYS_TD_PEND_CAP (896), else 64 .. GYS_TD_PEND_CAP_MAX.
	                              A batch's values of a service are appended while buffered + new <= td_pend_cap, otherwise ONE merge re-clusters
	                              the digest with all of them (and a service whose next batch of the same size would pass the fast merge size -- the
	                              smallest of 1024 / 2048 / 4096 values that is >= td_pend_cap + 128 -- is merged at once).  A merge costs almost the same whatever it carries (its work is per cluster and per value bin), so a
	                              larger buffer means proportionally fewer merges per window: 3968 at 54 values per service and window = a merge
	                              every ~70 windows instead of every ~17, for 4 x 3968 bytes more HBM per service.  The digest state is a function
	                              of the per-call value multisets AND of this number (the CPU oracle takes the same parameter). */
	uint32_t svc_hll_levels;   /* 1 = keep the per-service HyperLogLog registers of the CLOSED windows for the four levels (window closed last /
	                              300 s / 5 days / all; "distinct-flow counts of the closed windows" below); needs svc_hll_p.  22 register files per
	                              service: 352 B at svc_hll_p = 4 (3.5 GB at 10^7 services), 22.5 KB at 10.  0 = off: nothing is allocated and a
	                              window close enqueues what it always did */
	uint32_t actconn_pair_cap; /* N > 0: the ACTIVE_CONN_STATS rows are also kept in an exact table keyed by (listener, client task group, kind) with
	                              room for N live keys ("live active-connection rows" below; 2 x N entries, rounded up to a power of two, of 128
	                              bytes, in two buffers).  0 = off: nothing is allocated, gys_ingest_active_conns launches what it always did and
	                              the calls of that section answer GYS_ERR_STATE.  Not part of the service-record fingerprint: the table is not
	                              per-service state */
} gys_config;

/* -------------------------------------------------------------------------------------------------------------------
 * lifecycle */
uint32_t gys_abi_version(void);
const char *gys_last_error(void);
uint64_t gys_reduce_arena_bytes(const gys_config *cfg); /* size the caller must provide in cfg->reduce_arena */
int gys_create(const gys_config *cfg, gys_ctx **out);
void gys_destroy(gys_ctx *ctx);
int gys_sync(gys_ctx *ctx); /* hipStreamSynchronize on the context stream */

/* host-id shard function: GY_MACHINE_ID::get_hash() % nshards  (common/gy_sys_hardware.h:82-85) */
uint32_t gys_machine_id_hash(const uint8_t machine_id[16]);
uint32_t gys_shard_of(const uint8_t machine_id[16], uint32_t nshards);

/* -------------------------------------------------------------------------------------------------------------------
 * registration (control-plane facts the data path needs; the reference learns them from PM_CONNECT / NOTIFY_NEW_LISTENER,
 * server/gy_mconnhdlr.cc partha registration + handle_add_listener -- out of scope beyond these two calls) */
/* Cluster indices are assigned in first-seen order per context; in a multi-rank job call gys_register_cluster for every cluster
 * name in the SAME order on every rank before registering hosts, so that the all-reduced cluster rows line up. */
int gys_register_cluster(gys_ctx *ctx, const char *cluster_name, uint32_t *cluster_idx);
int gys_register_host(gys_ctx *ctx, const uint8_t machine_id[16], const char *cluster_name, uint32_t *host_slot);

typedef struct {
	uint64_t glob_id;   /* TCP_LISTENER::glob_id_ (opaque 64-bit id on the wire) */
	uint32_t netns;     /* network namespace inode as carried by the eBPF tuple (partha/gy_ebpf_kernel_struct.h:28-35) */
	uint16_t port;      /* listener port, host order */
	uint8_t is_any_ip;  /* comm::NEW_LISTENER::is_any_ip_ (common/gy_comm_proto.h:1539; TCP_LISTENER::is_any_ip_ = addr.is_any_address(),
	                       common/gy_socket_stat.cc:1796): non-zero = the listener takes the events of every address of its (netns, port) */
	uint8_t addr_is_v6; /* is_any_ip == 0: addr is an in6_addr (16 bytes) when non-zero, else an in_addr in addr[0..3] (network order) */
	char comm[16];      /* TASK_COMM_LEN process name (LISTEN_TOPN::comm_) */
	uint8_t addr[16];   /* is_any_ip == 0: the address the listener is bound to -- NEW_LISTENER::ns_ip_port_.ip_port_.ipaddr_.  A response event
	                       reaches the listener only when its server address equals this one the way GY_IP_ADDR::operator== compares
	                       (common/gy_common_inc.h:10629-10636: an IPv6 address that embeds an IPv4 one -- ::ffff:a.b.c.d, 2002::/16,
	                       64:ff9b::/32 -- equals that IPv4 address); ignored when is_any_ip != 0 */
} gys_listener_info;

/* Listener lookup of a response event (replaces listener_tbl_.lookup_single_elem(ser_nsipport, hash ignoring the IP) with the comparator
 * operator==(shared_ptr<TCP_LISTENER>, NS_IP_PORT), common/gy_socket_stat.cc:1671, common/gy_socket_stat.h:708-714): among the listeners
 * registered for the host with the event's (netns, server port), in registration order, the first one that is_any_ip or is bound to the
 * event's server address takes the event; if none does the event is dropped (gys_counters.resp_dropped_nolistener).  Registration follows
 * insert_or_replace (common/gy_socket_stat.cc:1372, :7779): a new listener REPLACES, in place, the first registered listener of its
 * (netns, port) that is_any_ip or is bound to the same address -- that listener's slot keeps its state but gets no further response events
 * -- and is appended behind the others otherwise. */

/* assigns consecutive service slots [*first_slot, *first_slot + n) to the listeners the engine does not know yet.  A glob_id that is
 * already registered (a partha resends its listeners after a reconnect) keeps its slot and all of its state, and repeats inside one call
 * are dropped: with such entries fewer than n slots are assigned (gys_lookup_service gives any listener's slot).
 * The slots come from the TAIL only -- [gys_num_services, max_services) -- and never from the free slots gys_delete_listeners left:
 * GYS_ERR_NOMEM at the tail's end even while free slots exist.  gys_register_listeners_slots takes those. */
int gys_register_listeners(gys_ctx *ctx, const uint8_t machine_id[16], const gys_listener_info *arr, uint32_t n, uint32_t *first_slot);

/* -------------------------------------------------------------------------------------------------------------------
 * deleting listeners.  The reference removes a listener from glob_listener_tbl_ and the partha's listen_tbl_ on a LISTENER_STATE_NOTIFY
 * record flagged LISTEN_FLAG_DELETE (server/gy_mconnhdlr.cc:11195-11248; the agent sends it when the listener goes away,
 * common/gy_socket_stat.cc:4021-4036) and synthesises such records every cleanup cycle for the listeners whose state is older than 30
 * minutes (server/gy_mconnhdlr.cc:16296-16343).  The engine's ingest only MARKS the kept state on such a record (its window word becomes 0,
 * gys_counters.lstate_deleted); the caller removes the service with the calls below -- gys_list_stale_listeners finds the marked and the
 * aged ones.
 *
 * gys_delete_listeners: every id is looked up before anything changes.  An id the engine does not know is neither counted in *ndeleted
 * (may be NULL) nor an error (the reference's nmissed); repeats inside the call count once.  GYS_ERR_INVAL for glob_ids == NULL with n != 0.
 * The call first puts whatever the three submission queues hold on the stream (as every call outside the host-pointer ingest does): what
 * was ingested before it is applied to the service before it goes.  On return -- device work follows in stream order --
 *   - gys_lookup_service(id) gives GYS_ERR_NOTFOUND; state / connection / active-connection records that name the id count as missed / unknown;
 *   - a response event for its (netns, port) is dropped (resp_dropped_nolistener) or goes to the next listener of that key by the
 *     first-match rule above;
 *   - the service's slot is a FREE SLOT: it belongs to no host (it has left the host's roll-ups, top-N and JSON lists), is in neither key
 *     table, has no label (GYS_NO_GROUP) and its per-service state is reset to what gys_create leaves -- buffered values, digest, both
 *     histogram records, bitmap rows, counters, kept state, level snapshots, distinct-count files, QPS / active-connection histograms.
 *     Every export, scan and window close is still sized by gys_num_services and writes for a free slot what it writes for a registered
 *     service that never got data (a close that goes by while the slot is free leaves it the first-close time of such a service);
 *     gys_register_listeners_slots resets a free slot once more when it hands it out, so a reused slot starts like a tail slot;
 *     gys_scan_listener_state_dev's records of a free slot carry glob_id 0; GYS_RF_ANY_STATE selections skip free slots;
 *   - the service's part of the OPEN window is discarded with it (its window event count, i.e. its Count-Min share at the close: the
 *     reference drops the object and its histograms the same way).  What already went into rank-wide registers stays: the global HLL,
 *     the all-service histogram, host summaries, cluster rows, pair Count-Mins. */
int gys_delete_listeners(gys_ctx *ctx, const uint64_t *glob_ids, uint32_t n, uint32_t *ndeleted);

/* gys_register_listeners with a slot per listener: slots[i] (may be NULL) = the slot of arr[i], new or known.  The rules are those of
 * gys_register_listeners (known ids keep their slot, repeats inside the call are dropped and report the first one's slot); new ids, in
 * array order, take FREE SLOTS first, lowest slot number first, and consecutive tail slots after that.  GYS_ERR_NOMEM only when free
 * slots and tail together do not suffice; nothing is registered then.  (A key-table insert that fails -- the tables are sized for
 * max_services at a load of 1/2, so this means a broken table -- also gives GYS_ERR_NOMEM, as in gys_register_listeners; the device side
 * of the call is then partly done and not undone, and the context should be destroyed.) */
int gys_register_listeners_slots(gys_ctx *ctx, const uint8_t machine_id[16], const gys_listener_info *arr, uint32_t n, uint32_t *slots);

/* free slots below gys_num_services (which stays the high-water mark every export and scan is sized by) */
uint32_t gys_num_free_slots(gys_ctx *ctx);

/* bytes of per-service device state in this context's configuration: what a delete resets per slot (the buffered values of the digest,
 * which need no reset behind a zero cursor, are not counted) */
uint64_t gys_svc_state_bytes(gys_ctx *ctx);

/* The reference's inactivity walk (server/gy_mconnhdlr.cc:16296-16343) as one device pass over the kept state records, plus the pick-up
 * of the delete records.  flags:
 *   GYS_STALE_DELETED  services whose kept record was marked by a LISTEN_FLAG_DELETE record (window word 0 under a non-zero id).  A
 *                      listener deleted before it ever reported state cannot be told from one that never reported and is NOT listed:
 *                      the caller has that id from the message itself;
 *   GYS_STALE_AGED     services whose kept record is older than max_age_windows closed windows: kept in window w with more than
 *                      max_age_windows windows closed since w opened (360 = the reference's 30 minutes of 5-s windows).
 * Services that never reported state and free slots are never listed.  *nfound = all hits and may exceed cap; the first `cap` ids in
 * ascending slot order are written to glob_ids (cap may be any number: the engine's id buffer is sized by min(cap, gys_num_services)).  Nothing is modified: the caller hands the ids to gys_delete_listeners.  Synchronous. */
#define GYS_STALE_DELETED 1u
#define GYS_STALE_AGED 2u
int gys_list_stale_listeners(gys_ctx *ctx, uint32_t flags, uint32_t max_age_windows, uint64_t *glob_ids, uint32_t cap, uint32_t *nfound);

/* -------------------------------------------------------------------------------------------------------------------
 * ingest
 *
 * Host-pointer entry points (gys_ingest_resp_events, gys_ingest_tcp_conn, gys_ingest_listener_state): the caller's buffer is only
 * read DURING the call (the reference's pone points into the L1 receive buffer, freed after the dispatch switch) and
 * the call does NOT wait for the GPU: the records are copied into a slot of a ring of 16 pinned staging buffers (handed out oldest
 * first), one H2D copy and the ingest kernels are enqueued, and the call returns; a slot is reused once the event recorded behind its
 * kernels has fired (gys_counters.stage_waits counts the calls that had to wait for that) -- this is the path of
 * gys_ingest_active_conns and of a connection / listener-state call of many messages' size (> 8 MiB / 2 MiB of records).  A partha's
 * TCP_CONN_NOTIFY and LISTENER_STATE_NOTIFY messages (gys_ingest_tcp_conn, gys_ingest_listener_state) go through SUBMISSION QUEUES of
 * their own: the messages of all threads are appended to one pinned batch (records + an offset and the sender's host slot per record)
 * that is copied and launched once; records keep the order in which the calls arrived, so the last state record of a listener wins
 * across the messages of a batch as it does across calls (gys_counters.conn_calls_queued / conn_submissions, lstate_*).
 * gys_ingest_resp_events goes through a SUBMISSION QUEUE as well: the calls of all threads are concatenated into one pinned batch (a segment per call) and handed to the
 * response pipeline together -- with an idle GPU a call is submitted at once; while two submissions are still executing, further calls
 * accumulate and go out together as soon as one of them has finished (group commit: the fixed launches of a response batch are paid
 * once per submission exactly when the GPU is the bottleneck; a host appears at most once per combined batch and batches are submitted in the order they were
 * sealed, so every service sees its per-call value multisets in call order and the state is bit-identical to per-call ingestion).
 * A call may therefore return before its events are on the stream; every other entry point puts the queue's content on the stream first.
 * These three calls may be made concurrently from several threads (up to the reference's MAX_L2_MISC_THREADS = 16,
 * server/gy_mconnhdlr.h:60) on the same context.  Everything else -- registration, the _dev entry points, the wire front end, the
 * window boundary, queries and exports -- must not run concurrently with any other call on the context (gys_mconn_shim.hpp holds a
 * shared / exclusive lock accordingly).  Results become visible to queries in stream order; gys_sync waits for them. */

/* Raw response events in the eBPF layout tcp_ipv4_resp_event_t (common/gy_ebpf_kernel.h:106-111, 24 bytes: saddr,daddr,netns,
 * sport,dport (network order), lsndtime, lrcvtime).  Replaces TCP_SOCK_HANDLER::handle_ipv4_resp_event + handle_tcp_resp_event
 * (common/gy_socket_stat.cc:1517-1677): per event RESP_TIME_HASH bucket + histogram add + CONN_BITMAP + query count, plus the new
 * t-digest / HLL / CMS sketches. */
int gys_ingest_resp_events(gys_ctx *ctx, const uint8_t machine_id[16], const void *ev24, uint32_t nevents);

typedef struct {
	uint32_t host_slot;   /* from gys_register_host */
	uint32_t reserved;    /* ignored on input (the engine clears its copy; it uses the field for its own per-part segment lists) */
	uint64_t first_event; /* index of this host's first event; segments sorted ascending, host's events contiguous */
} gys_resp_seg;

/* device-resident multi-host batch: d_ev24 is a DEVICE pointer to nevents 24-byte events; segs is a HOST array */
int gys_ingest_resp_events_dev(gys_ctx *ctx, const gys_resp_seg *segs, uint32_t nsegs, const void *d_ev24, uint64_t nevents);

/* IPv6 response events in the eBPF layout tcp_ipv6_resp_event_t (common/gy_ebpf_kernel.h:113-118, 48 bytes: ipv6_tuple_t
 * {u128 saddr, u128 daddr, u32 netns, u16 sport, u16 dport (network order)} partha/gy_ebpf_kernel_struct.h:37-44, then lsndtime, lrcvtime).
 * Replaces TCP_SOCK_HANDLER::handle_ipv6_resp_event (common/gy_socket_stat.cc:1535-1551) -> handle_tcp_resp_event(is_ipv4 = false): the same
 * filter, listener lookup and RESP_TIME_HASH bucket as the IPv4 form; the histogram and the query count are the listener's shared ones
 * (resp_cache_v6_ flushes into the same resp_hist_, :1800; curr_query_v4_ + curr_query_v6_, :4050-4051), the CONN_BITMAP rows are the
 * listener's resp_bitmap_v6_ (:1587; rows 32..63 of gys_export_conn_bitmap, added to the IPv4 rows' counts per bucket as :4144-4149 does).
 * Flow key: PAIR_IP_PORT(daddr:dport, saddr:sport) with both addresses through GY_IP_ADDR(unsigned __int128) -- an address that embeds an
 * IPv4 one hashes and compares as that IPv4 address (common/gy_common_inc.h:11040-11129, :10950-10959).  The reference has one perf buffer and
 * one handler thread per family (PROBE_TCP_RESPONSE_IPv4 / _IPv6, common/gy_socket_stat.cc:101-102): a stream is handed over as calls of
 * one family each.  The host-pointer form is its own submission (it does not join the IPv4 submission queue, it runs behind it). */
int gys_ingest_resp_events_v6(gys_ctx *ctx, const uint8_t machine_id[16], const void *ev48, uint32_t nevents);
int gys_ingest_resp_events_v6_dev(gys_ctx *ctx, const gys_resp_seg *segs, uint32_t nsegs, const void *d_ev48, uint64_t nevents);

/* Replaces MCONN_HANDLER::partha_tcp_conn_info(partha, TCP_CONN_NOTIFY *pone, int nconns, uint8_t *pendptr, ...)
 * (server/gy_mconnhdlr.h:2091, .cc:9052-9444): flow key PAIR_IP_PORT(nat_cli_, nat_ser_) (.cc:8707) -> distinct-flow HLL;
 * per-service connection / byte counters (connlistenmap_ roll-up .cc:9133-9319) -> exact per-service counters + CMS.
 * The batch is walked like the reference's L2 loop `for (i < nconns && p < pendptr; p += get_elem_size())` (.cc:9130, :11175) under the
 * L1 validators' rule (TCP_CONN_NOTIFY::validate / LISTENER_STATE_NOTIFY::validate, common/gy_comm_proto.cc:859-880, :974-995: the L2
 * loop only ever sees messages that passed it): every one of the nconns announced records lies complete before `pend` and has a size
 * that is a multiple of 8; otherwise GYS_ERR_INVAL and nothing of the batch is ingested.  `pend` must not be NULL.  (The wire front end
 * gys_ingest_comm_stream applies the same rule on the GPU.) */
int gys_ingest_tcp_conn(gys_ctx *ctx, const uint8_t machine_id[16], const void *batch, uint32_t nconns, const void *pend);
/* device-resident: d_offsets[i] = byte offset of record i inside d_batch (records are variable stride: get_elem_size()) */
int gys_ingest_tcp_conn_dev(gys_ctx *ctx, const void *d_batch, const uint32_t *d_offsets, uint32_t nconns);

/* Replaces MCONN_HANDLER::partha_listener_state(partha, const LISTENER_STATE_NOTIFY *pone, int nconns, uint8_t *pendptr, ...)
 * (server/gy_mconnhdlr.h:2129, .cc:10993-11412): per record glob_id probe, LISTEN_SUMM_STATS::update, set_state, top-N. */
int gys_ingest_listener_state(gys_ctx *ctx, const uint8_t machine_id[16], const void *batch, uint32_t nrecs, const void *pend);

/* Wire front-end: a byte stream of COMM_HEADER-framed messages exactly as an unmodified partha sends them on its PM_HDR_MAGIC
 * connection ([COMM_HEADER 16 B][EVENT_NOTIFY 8 B][nevents_ records][padding], common/gy_comm_proto.h:336-420, :486-500).
 * Replaces the L1 validation + L2 dispatch in front of the two handlers above (COMM_HEADER::validate common/gy_comm_proto.cc:10-57,
 * TCP_CONN_NOTIFY::validate :840-881, LISTENER_STATE_NOTIFY::validate :955-996, dispatch server/gy_mconnhdlr.cc:4756-4792): message
 * headers are checked on the host, the variable-stride record chains are walked, checked and indexed ON THE GPU (pointer doubling +
 * prefix sum, gys_kernels.hpp "wire front-end"), EVENT_NOTIFY subtypes NOTIFY_TCP_CONN / NOTIFY_LISTENER_STATE are ingested, every
 * other message is skipped (control plane).  A malformed header or record rejects the call (the reference drops the connection);
 * nothing of the rejected call is ingested for the kind that failed.  buf must be 8-byte aligned. */
typedef struct {
	uint32_t nmsgs, nmsgs_tcp_conn, nmsgs_listener_state, nmsgs_skipped, nmsgs_invalid, reserved;
	uint64_t nrecords;       /* TCP_CONN_NOTIFY + LISTENER_STATE_NOTIFY records ingested */
	uint64_t bytes_consumed; /* whole messages consumed; a trailing partial message is left to the caller */
} gys_comm_stats;
int gys_ingest_comm_stream(gys_ctx *ctx, const uint8_t machine_id[16], const void *buf, uint64_t nbytes, gys_comm_stats *out);
/* device-resident multi-host: d_host_slot[i] = host of record i */
int gys_ingest_listener_state_dev(gys_ctx *ctx, const void *d_batch, const uint32_t *d_offsets, const uint32_t *d_host_slot,
				  uint32_t nrecs);

/* Replaces MCONN_HANDLER::handle_partha_active_conns(partha, const comm::ACTIVE_CONN_STATS *pconn, int nitems, uint8_t *pendptr, ...)
 * (server/gy_mconnhdlr.h:2039, .cc:7705-7772; rows comm::ACTIVE_CONN_STATS common/gy_comm_proto.h:2766-2783, 104-byte fixed stride, a
 * partha's 15-s report of (listener, client task group) rows).  The reference formats every row into an SQL insert
 * (insert_active_conns .cc:7776-7960: is_remote_listen_ == false -> activeconntbl, true -> remoteconntbl).  Here the local-listener
 * rows update (i) a Count-Min pair keyed by (listener_glob_id_, cli_aggr_task_id_): active_conns_ (u32 table) and bytes_sent_ +
 * bytes_received_ (u64 table) -- the per-(listener, client task) roll-up that stands for those rows; both tables live in the reduce
 * arena (all-reduced with the other registers, per window; queries read the per-cell maximum of the last three windows' tables, see
 * gys_query_pair_cms) -- and (ii) exact cumulative per-listener sums.  Remote-listener rows (is_remote_listen_: the listener lives on another
 * madhava, server/gy_mconnhdlr.cc:7888-7925 -> remoteconntbl) are rolled up the same way into a Count-Min pair of their own (gys_query_pair_cms
 * which 6 / 7) and counted (gys_counters.actconn_remote_listen); they name no service of this engine, so there are no per-listener sums for them.
 * A Count-Min can only be asked about a pair the caller already knows: with gys_config.actconn_pair_cap the rows of both kinds are also kept,
 * exactly, in a keyed table that can be enumerated ("Live active-connection rows" below). */
int gys_ingest_active_conns(gys_ctx *ctx, const uint8_t machine_id[16], const void *batch, uint32_t nitems, const void *pend);
int gys_ingest_active_conns_dev(gys_ctx *ctx, const void *d_batch, uint32_t nitems);

typedef struct {
	uint32_t ntasks_issue, ntasks, nlisten_issue, nlisten; /* comm::HOST_STATE_NOTIFY fields used by update_from_state */
	uint8_t cpu_issue, mem_issue, curr_state, reserved;
} gys_host_state;
/* Replaces the host_state_ store read by MCONN_HANDLER::send_cluster_state (server/gy_mconnhdlr.cc:16052-16075) */
int gys_ingest_host_state(gys_ctx *ctx, const uint8_t machine_id[16], const gys_host_state *st);

/* -------------------------------------------------------------------------------------------------------------------
 * window boundary (the reference's 5 s cadence: send_cluster_state -> handle_cluster_state -> aggregate_cluster_state,
 * server/gy_mconnhdlr.cc:16052, server/gy_shconnhdlr.cc:4554-4640)
 *
 *   gys_window_prepare : local roll-ups are written into the reduce arena (cluster STATE_ONE sums, global histogram, HLL, CMS)
 *   <caller all-reduces every gys_reduce_section across ranks: RCCL over xGMI, or nothing for a single GPU>
 *   gys_window_finish  : consumes the reduced arena (global answers), folds window histograms into the all-time ones,
 *                        clears window state.
 */
typedef struct {
	void *dev_ptr;
	uint64_t nelems;
	uint32_t dtype; /* 0 = u8, 1 = u32, 2 = i64 */
	uint32_t op;    /* 0 = MAX, 1 = SUM */
} gys_reduce_section;

int gys_reduce_sections(gys_ctx *ctx, gys_reduce_section out[4], uint32_t *nsections);
int gys_window_prepare(gys_ctx *ctx, uint64_t tusec);
int gys_window_finish(gys_ctx *ctx);
/* single rank: gys_window_prepare + gys_window_finish as ONE captured hipGraph (the fold kernels that are due, k_window_prepare, the
 * copy / clear sequence, the window-number increment), captured once per registry shape and replayed with one launch per window
 * (gys_counters.window_graph_launches).  Falls back to the two calls with multi-level windows or nranks > 1 (gys_window_close_rccl). */
int gys_window_close(gys_ctx *ctx, uint64_t tusec);

/* -------------------------------------------------------------------------------------------------------------------
 * queries (result shapes: common/gy_json_field_maps.h svcsumm :1396-1416, clusterstate :2162-2180, svcstate :1102-1135) */

typedef struct {
	int32_t nstates[GYS_NSTATES];
	int32_t tot_qps, tot_act_conn, tot_kb_inbound, tot_kb_outbound, tot_ser_errors, nlisteners, nactive;
} gys_svcsumm; /* == LISTEN_SUMM_STATS<int>, server/gy_msocket.h:840-851 */

typedef struct {
	uint32_t nhosts, ntasks_issue, ntaskissue_hosts, ntasks, nsvc_issue, nsvcissue_hosts, nsvc, total_qps, svc_net_mb,
		ncpu_issue, nmem_issue;
} gys_cluster_state; /* == comm::MS_CLUSTER_STATE::STATE_ONE, common/gy_comm_proto.h:3183-3197 */

typedef struct {
	int64_t data_value; /* bucket ceiling, get_bucket_max_threshold (common/gy_statistics.h:500-515) */
	int64_t sum;
	uint64_t count;
	float percentile;
	uint32_t reserved;
} gys_hist_data; /* == HIST_DATA, common/gy_statistics.h:473-484 */

typedef struct {
	uint64_t count;
	int64_t sum;
} gys_hist_serial; /* == HIST_SERIAL, common/gy_statistics.h:458-468 */

typedef struct {
	gys_hist_serial stats[GYS_MAX_BUCKETS - 1]; /* 15 buckets */
	uint64_t total_count;
	int64_t max_val_seen;
} gys_hist_rec; /* 256 bytes: the arithmetic state of GY_HISTOGRAM<int64_t,RESP_TIME_HASH> (280 B incl. clocks) */

int gys_query_svcsumm(gys_ctx *ctx, const uint8_t machine_id[16], gys_svcsumm *out);      /* web_curr_listener_summ, gy_mnodehandle.cc:1628 */
int gys_query_clusterstate(gys_ctx *ctx, const char *cluster_name, gys_cluster_state *out); /* aggregate_cluster_state result */
/* GY_HISTOGRAM::get_percentiles (common/gy_statistics.h:707-791) of one service; which: 0 = current (open) window, 1 = all-time.
 * "All-time" is every response ingested so far INCLUDING the open window, in both record modes (t-digest on: lazily folded records;
 * off: per-event records, window added at the boundary) -- the same answer mid-window whichever mode runs (tests/test_gpu_resp.py).
 * The same `which` applies to gys_scan_percentiles_dev and gys_export_hist. */
int gys_query_hist_percentiles(gys_ctx *ctx, uint64_t glob_id, int which, gys_hist_data *pdata, uint32_t npct, uint64_t *total_count,
			       int64_t *max_val, float *pavg);
/* t-digest quantiles (q in [0,1]) of one service's response times: computed from the merged view (clusters re-clustered with the
 * values the key still buffers; the stored state is not modified), rounded half-up to whole milliseconds */
int gys_query_quantiles(gys_ctx *ctx, uint64_t glob_id, const double *q, uint32_t nq, double *out);
/* distinct flows seen (global HLL over PAIR_IP_PORT keys; after gys_window_finish: the all-rank estimate) */
int gys_query_distinct_flows(gys_ctx *ctx, double *out);
/* Count-Min estimate for a service key in the last finished window: which = 0 response events + NEW CONNECTIONS of the service (one per
 * connection, accepting side: see gys_export_svc_counters), which = 1 connection bytes (sent + received) */
int gys_query_cms(gys_ctx *ctx, uint64_t glob_id, int which, uint64_t *out);
/* Count-Min estimate for a (listener, client task group) pair.  Two roll-ups, each with its own table pair:
 *   which 0 / 1: active connections / bytes (sent + received) of the ACTIVE_CONN_STATS rows (gys_ingest_active_conns).  A partha reports
 *                these every 15 s on a phase of its own and a window is 5 s: the answer is the PER-CELL MAXIMUM over the (all-rank) tables
 *                of the last three finished windows -- a pair reported anywhere in the last 15 s reads back at least its reported value
 *                (Count-Min never under-estimates), a partha whose report fell into two of the three windows is not counted twice, and a
 *                pair not reported for three windows reads 0 again (a gauge's "last report").
 *   which 2 / 3: closed connections / their bytes of the TCP_CONN_NOTIFY roll-up, LISTENER side = the reference's connlistenmap_
 *                (server/gy_mconnhdlr.cc:9226-9245: records with tusec_close_, bytes > 0, ser_glob_id_ and is_tcp_accept_event_), last
 *                finished window (gys_config.conn_pair_cms; GYS_ERR_STATE when off);
 *   which 4 / 5: the same for the CLIENT side = connclientmap_ (:9290-9312: closed, bytes > 0, connect-only, cli_task_aggr_id_ != 0). */
int gys_query_pair_cms(gys_ctx *ctx, uint64_t listener_glob_id, uint64_t cli_aggr_task_id, int which, uint64_t *out);

typedef struct {
	uint64_t glob_id;
	uint32_t host_slot;
	uint32_t metric; /* the ranked value */
	uint8_t state[88]; /* the LISTENER_STATE_NOTIFY record (common/gy_comm_proto.h:2183-2254) as last ingested */
} gys_topn_entry;
/* per-host top-N of the last window by kind: 0 issue, 1 qps, 2 active conns, 3 net (LISTEN_TOPN comparators gy_msocket.h:720-796) */
int gys_query_topn(gys_ctx *ctx, const uint8_t machine_id[16], int kind, gys_topn_entry out[GYS_TOPN], uint32_t *nout);

/* The "per-key scan" (TCP_SOCK_HANDLER::listener_stats_update percentile part, common/gy_socket_stat.cc:4226-4230) over ALL services
 * on the GPU: for service slot s and percentile i, d_out[s*npct + i] = bucket ceiling; which as above.  d_out is a DEVICE pointer. */
int gys_scan_percentiles_dev(gys_ctx *ctx, int which, const float *pcts, uint32_t npct, int64_t *d_out);
/* the same scan on the t-digests: quantile q[i] (0..1, nq <= 16) of EVERY service's merged view (clusters re-clustered with the buffered
 * values; no state is modified), d_out[slot * nq + i] on the device -- identical, value for value, to gys_query_quantiles of that service.
 * Replaces the per-listener p25 / p95 / p99 search of TCP_SOCK_HANDLER::listener_stats_update (common/gy_socket_stat.cc:4044-4365,
 * percentile calls :4226-4230) for all listeners at once.  q is a HOST array, d_out a DEVICE pointer to nsvc * nq doubles. */
int gys_scan_quantiles_dev(gys_ctx *ctx, const double *q, uint32_t nq, double *d_out);

/* -------------------------------------------------------------------------------------------------------------------
 * Ranks: how many responses finished within x ms -- the inverse of the quantile calls, for the share of requests inside a latency
 * objective (below / total), an error budget or an Apdex figure, per service and per group.  Builder-defined, PARITY UNPINNED like the
 * t-digest itself.  The definition is FROZEN.  For a digest with clusters {sum[k], cnt[k]} (k < GYS_TD_NB), extremes vmin / vmax, a
 * multiset P of buffered values (a service's; empty for a slab) and an integer threshold x (milliseconds, any int64_t), below(x) is a
 * double that estimates the number of recorded values <= x:
 *   1. nb = the number of values of P that are <= x: exact.
 *   2. N = sum of cnt; total = N + |P|.  N = 0: below = (double)nb.
 *   3. lo = min(vmin, min P), hi = max(vmax, max P).  x < lo: the clusters' part r = 0.  x >= hi: r = (double)N.
 *   4. Otherwise the clusters are read at y = (double)x + 0.5: the values are whole milliseconds, and a value v stands for the interval
 *      [v - 1/2, v + 1/2] -- the inverse of the quantile calls, which round the interpolated latency half-up to whole milliseconds.  Over the
 *      non-empty clusters in index order, W_k = the exact integer weight before cluster k, c_k = (double)W_k + (double)cnt_k * 0.5,
 *      m_k = (double)sum_k / (double)cnt_k; j = the greatest non-empty index whose mean is at most x + 1/2, decided in exact integers:
 *      sum_j - floor(cnt_j / 2) <= x * cnt_j (128-bit product); n = the next non-empty index after j, f = the first non-empty index:
 *        no such j:     r = c_f * ((y - ((double)lo - 0.5)) / (m_f - ((double)lo - 0.5)))
 *        j is the last: r = c_j + ((double)N - c_j) * ((y - m_j) / (((double)hi + 0.5) - m_j))
 *        otherwise:     r = c_j + (c_n - c_j) * ((y - m_j) / (m_n - m_j))
 *      Every denominator is positive by construction.  Only + - * / on doubles, in exactly this order (the library is built with
 *      -ffp-contract=off: a restatement in another language gives the same bits).
 *   5. below = r + (double)nb.
 * The buffered values are counted exactly, not merged virtually.  below is monotone in x, 0 for x below every value and == total at and
 * above the largest.  Why x + 1/2 and not x: read at x itself, a cluster whose mean is exactly x counts with half its weight (its centre)
 * although all of its values are <= x; wherever one millisecond value carries a hundredth of the weight (a service answering in 1 500 +- 3 ms,
 * the small latencies of a lognormal) that alone was 1.0 - 1.5 % of the total, above the project's 1 % rank-error tolerance.  Measured rank
 * error |below - exact| / total against the exact sort: DESIGN.md section 4.
 * thr is a HOST array of nt = 1 .. 16 thresholds (GYS_ERR_INVAL otherwise); GYS_ERR_STATE when enable_tdigest is 0.  No state is modified. */
/* one service: below[nt] and *total (may be NULL) on the HOST */
int gys_query_ranks(gys_ctx *ctx, uint64_t glob_id, const int64_t *thr, uint32_t nt, double *below, uint64_t *total);
/* EVERY service slot in one streaming pass: d_below[slot * nt + i], d_total[slot] (DEVICE; d_total may be NULL).  A slot without data and
 * a free slot give 0 and 0.  Row `slot` equals gys_query_ranks of that service bit for bit.  Asynchronous on the context stream (gys_sync). */
int gys_scan_ranks_dev(gys_ctx *ctx, const int64_t *thr, uint32_t nt, double *d_below /* [nsvc * nt] */, uint64_t *d_total /* [nsvc] */);

/* -------------------------------------------------------------------------------------------------------------------
 * Roll-up digests: the response-time digest of a GROUP of services -- a host, a cluster, all hosts of this rank ("global") -- and the
 * merge of such digests across ranks.  Replaces the aggregated percentile Postgres computes over a set of listeners' rows,
 * public.tdigest_percentile(col, 100, p) (common/gy_query_common.cc:1818-1855), and feeds the fan-in of
 * SHCONN_HANDLER::aggregate_cluster_state (server/gy_shconnhdlr.cc:4583-4720).  Definition (oracle/gy_oracle_rollup.c, gyo_tdbins_*; round 6:
 * no longer an ordered fold): the UNION BY VALUE BIN -- every member's non-empty clusters go, whole, into the value bin (one per millisecond
 * below 1024, 64 cells per octave above) of the integer threshold of their mean, a service's buffered values into the bin of the value; the
 * bins' exact 64-bit {sum, count} are then laid on the rank axis in order and cut into the 200 clusters by the engine's cluster rule, a bin
 * that spans a cluster boundary sharing its sum in proportion (exact integers).  A bin of 1024 ms and above that a boundary cuts and that
 * holds more than 1 / 1024 of the weight is refined first: a second pass over the members puts its share into up to 1920 / (refined bins)
 * cells of equal width (down to 1 ms), which take the bin's place in the layout.  The result does not depend on the order of the members.  A
 * roll-up digest as a member contributes its clusters the same way.  Fixed-size slab = the unit a multi-rank job all-gathers (ncclAllGather
 * of sizeof(gys_tdigest_slab) bytes per rank) and rolls up with gys_tdigest_merge_slabs_dev. */
typedef struct {
	int64_t sum[GYS_TD_NB];
	uint64_t cnt[GYS_TD_NB];
	int64_t vmin, vmax; /* valid when any cnt != 0 */
} gys_tdigest_slab;
enum { GYS_ROLLUP_HOST = 0, GYS_ROLLUP_CLUSTER = 1, GYS_ROLLUP_GLOBAL = 2 };
/* d_out (DEVICE): HOST: one slab per host slot [gys_num_hosts] -- the roll-up of the host's services; CLUSTER: one per registered cluster
 * index -- the roll-up of its hosts' slabs; GLOBAL: one slab -- the roll-up of all host slabs of this rank.  No engine state is modified (the
 * hosts' member lists are kept on the device between calls and rebuilt after a registration). */
int gys_tdigest_rollup_dev(gys_ctx *ctx, int scope, gys_tdigest_slab *d_out);
/* d_out[0] (DEVICE) = roll-up of the slabs d_in[0..n) (the cross-rank merge after an all-gather; also any caller-defined group) */
int gys_tdigest_merge_slabs_dev(gys_ctx *ctx, const gys_tdigest_slab *d_in, uint32_t n, gys_tdigest_slab *d_out);
/* quantiles q[i] (0..1) of one DEVICE slab into the HOST array out (same interpolation and rounding as gys_query_quantiles) */
int gys_tdigest_slab_quantiles(gys_ctx *ctx, const gys_tdigest_slab *d_slab, const double *q, uint32_t nq, double *out);
/* the same for nslabs DEVICE slabs in one launch: d_out[i * nq + t] (DEVICE) equals, bit for bit, what gys_tdigest_slab_quantiles(ctx,
 * d_slabs + i, q + t, 1, ...) returns -- the same clamp of q to 0 .. 1, the same interpolation between the centres W_k + cnt_k / 2 of the
 * non-empty clusters, vmin / vmax at the ends, floor(r + 0.5), 0 for an empty slab.  The one-slab call adds the weights before a cluster up
 * in doubles, this one in exact integers converted once: the same numbers while a slab weighs less than 2^53 (every slab the engine can
 * produce is far below that).  q is a HOST array of nq = 1 .. 16 quantiles (GYS_ERR_INVAL otherwise).  Asynchronous on the context stream
 * (gys_sync); no state is modified. */
int gys_tdigest_slab_quantiles_dev(gys_ctx *ctx, const gys_tdigest_slab *d_slabs, uint32_t nslabs, const double *q /* HOST */, uint32_t nq,
				   double *d_out /* DEVICE [nslabs * nq] */);
/* below(x) ("Ranks" above; P is empty, the extremes are the slab's) of nslabs DEVICE slabs -- the host, cluster and global roll-ups, the rows
 * of gys_rollup_filtered_dev, a cross-rank merge: d_below[i * nt + t], d_total[i] = the slab's weight (DEVICE; d_total may be NULL).
 * Asynchronous on the context stream. */
int gys_tdigest_slab_ranks_dev(gys_ctx *ctx, const gys_tdigest_slab *d_slabs, uint32_t nslabs, const int64_t *thr, uint32_t nt, double *d_below,
			       uint64_t *d_total);
uint32_t gys_num_clusters(gys_ctx *ctx);

/* -------------------------------------------------------------------------------------------------------------------
 * Distinct-flow counts per service, host, cluster and rank from the per-service HyperLogLog registers (gys_config.svc_hll_p = 4 .. 10;
 * GYS_ERR_STATE when it is 0).  Definitions (oracle/gy_oracle.h: gyo_hll_merge, gyo_hll_estimate):
 *   a register FILE is 1 << svc_hll_p bytes, byte i = the largest rank seen for register i (one row of gys_export_svc_hll);
 *   the file of a GROUP (a host = its services, a cluster = its hosts, global = all hosts of this rank, any list of files) is the
 *   byte-wise maximum of its members' files; it does not depend on their order; without members, or without events: all zero;
 *   the ESTIMATE of a file is Flajolet's raw estimator alpha m^2 / sum 2^-rank, and linear counting m ln(m / zeros) when the raw value
 *   is <= 2.5 m and a register is zero.  The all-zero file gives exactly 0.  It is a function of the file's bytes alone: the per-service
 *   scan, the one-service query and the roll-ups return bit-identical doubles for identical files.
 * THE OPEN WINDOW: every call reads the per-service registers as gys_export_svc_hll returns them at the same moment -- the window being
 * filled; closing a window clears them (ask before the close, as for gys_scan_listener_state_dev; the closed windows are kept by
 * gys_config.svc_hll_levels, see below) -- and modifies no engine state.
 * DEVICE pointers to files must be 16-byte aligned (any device allocation is).  Asynchronous on the context stream like the other
 * *_dev calls (gys_sync to wait), except gys_query_distinct and gys_hll_global_rccl, which return when the result is there. */
/* the estimate of EVERY registered service in one pass: d_out (DEVICE) [gys_num_services] doubles */
int gys_scan_distinct_dev(gys_ctx *ctx, double *d_out);
/* one service, result in HOST memory: the same device code on one slot, bit-identical to that slot of gys_scan_distinct_dev.
 * GYS_ERR_INVAL for an unknown glob_id */
int gys_query_distinct(gys_ctx *ctx, uint64_t glob_id, double *out);
/* bytes of one register file of this context (1 << svc_hll_p; 0 when svc_hll_p is 0) */
uint32_t gys_hll_file_bytes(gys_ctx *ctx);
/* group files and / or their estimates; scope = GYS_ROLLUP_HOST: one per host slot [gys_num_hosts]; _CLUSTER: one per registered cluster
 * [gys_num_clusters]; _GLOBAL: one.  d_regs (DEVICE, ngroups * gys_hll_file_bytes) and d_est (DEVICE, ngroups doubles): either may be
 * NULL, not both.  The hosts' member lists are those of gys_tdigest_rollup_dev (kept on the device, rebuilt after a registration). */
int gys_hll_rollup_dev(gys_ctx *ctx, int scope, uint8_t *d_regs, double *d_est);
/* the union of the n files d_in (DEVICE, contiguous, not overlapping the outputs) into d_out[0] and / or its estimate into d_est[0]
 * (either may be NULL, not both): the cross-rank step after an all-gather, or any caller-defined group */
int gys_hll_merge_files_dev(gys_ctx *ctx, const uint8_t *d_in, uint32_t n, uint8_t *d_out, double *d_est);

/* -------------------------------------------------------------------------------------------------------------------
 * Distinct-flow counts of the CLOSED windows for the four levels of the histograms (gys_config.svc_hll_levels = 1; GYS_ERR_STATE when it is
 * 0; level 0 .. 3 as for gys_query_hist_level_stats, GYS_ERR_INVAL otherwise).  Builder-defined like the open-window calls above; the ring
 * arithmetic is that of the histogram levels, so both kinds of level expire at the same second.  Definition, with ring = GYS_LEVEL_RING = 10,
 * dur[1] = 300 s, dur[2] = 432000 s, idx(t, dur) = (t % dur) * ring / dur the bucket that holds second t, and start(t, dur, j) the most
 * recent start <= t of bucket j:
 *   STATE per service, next to the open window's file: `last` (the window closed last), ringfile[l][j] for l = 1, 2 and j = 0 .. 9 (the union
 *   of the windows whose close time fell into bucket j of level l while that bucket was live), `all` (every closed window); and one close time
 *   t_last per context (seconds, -1 = no close yet).
 *   CLOSE at tusec (gys_window_finish, gys_window_close, gys_window_close_rccl; the time is the one given to the prepare step), tnow =
 *   max(tusec / 10^6, t_last): for each l, every bucket j with t_last >= 0 and start(tnow, dur[l], j) > t_last is cleared, then
 *   ringfile[l][idx(tnow, dur[l])] = max(itself, open); all = max(all, open); last = open; open = 0; t_last = tnow.  Once per window.
 *   LEVEL FILE of a service at query time tusec, tq = max(tusec / 10^6, t_last):
 *     level 0      `last` if t_last >= 0 and tq - t_last < 5, else all zero;
 *     level 1, 2   the byte-wise maximum of the buckets j for which NOT start(tq, dur[l], j) > t_last
 *                  (equivalently, with w = dur / 10: the window closed at t_k belongs to the level iff t_k / w > tq / w - 10);
 *     level 3      `all`.
 *   Never the open window, and no query modifies state.  A GROUP's level file is the byte-wise maximum of its members' level files; the
 *   ESTIMATE of a file is the one defined above (the same bits for the same bytes).  Because the maximum is idempotent and commutative, a
 *   level file equals the file all flow keys of its member windows would leave in one empty file: the ring loses nothing.
 * A service registered after some closes has all-zero files for the windows before its registration.
 * No collective of its own: the cross-rank count of a level is gys_hll_rollup_level_dev(GYS_ROLLUP_GLOBAL) -> the caller's all-gather of
 * one file per rank -> gys_hll_merge_files_dev. */
/* the level's estimate of EVERY registered service: d_out (DEVICE) [gys_num_services] doubles; asynchronous */
int gys_scan_distinct_level_dev(gys_ctx *ctx, int level, uint64_t tusec, double *d_out);
/* one service, result in HOST memory: the same device code on one slot, bit-identical to that slot of gys_scan_distinct_level_dev.
 * GYS_ERR_INVAL for an unknown glob_id */
int gys_query_distinct_level(gys_ctx *ctx, uint64_t glob_id, int level, uint64_t tusec, double *out);
/* host / cluster / rank files and / or estimates of a level: scopes, outputs and NULL rules of gys_hll_rollup_dev.  The level's files of
 * all services are written once into a scratch array (gys_num_services files, kept by the context), then rolled up by the same launches */
int gys_hll_rollup_level_dev(gys_ctx *ctx, int scope, int level, uint64_t tusec, uint8_t *d_regs, double *d_est);

/* -------------------------------------------------------------------------------------------------------------------
 * The window exchange inside the library (RCCL over xGMI; no torch, no caller-written collective).  Replaces
 * MCONN_HANDLER::send_cluster_state -> SHCONN_HANDLER::aggregate_cluster_state (server/gy_mconnhdlr.cc:16052-16118,
 * server/gy_shconnhdlr.cc:4583-4720): one process per GPU, every rank calls gys_window_close_rccl at the 5-s boundary.
 * The communicator handle is an ncclComm_t carried as void* (no RCCL type in this header); a caller that already owns one
 * (e.g. from its own ncclCommInitRank) may pass it directly.  One node: gys_rccl_unique_id / gys_rccl_comm_create set
 * NCCL_SOCKET_IFNAME=lo unless the environment already names an interface (the bootstrap rendezvous then runs over loopback). */
#define GYS_RCCL_UID_BYTES 128
int gys_rccl_unique_id(uint8_t uid[GYS_RCCL_UID_BYTES]);                        /* rank 0: ncclGetUniqueId; hand the bytes to every rank */
int gys_rccl_comm_create(gys_ctx *ctx, const uint8_t uid[GYS_RCCL_UID_BYTES], int nranks, int rank, void **comm); /* ncclCommInitRank on ctx's device */
int gys_rccl_comm_destroy(void *comm);
/* gys_window_prepare, then the four register families of gys_reduce_sections all-reduced in place (u8 MAX, u32 SUM, i64 SUM, i64 MAX)
 * as ONE ncclGroup on the context stream, then gys_window_finish.  Asynchronous like every other call (gys_sync to wait). */
int gys_window_close_rccl(gys_ctx *ctx, void *comm, uint64_t tusec);
/* the global response-time digest across ranks: this rank's GYS_ROLLUP_GLOBAL slab, ncclAllGather of the fixed-size slabs, their
 * roll-up (gys_tdigest_merge_slabs_dev) into d_out[0] (DEVICE) -- the same slab on every rank */
int gys_tdigest_global_rccl(gys_ctx *ctx, void *comm, gys_tdigest_slab *d_out);
/* the distinct-flow count across ranks: this rank's GYS_ROLLUP_GLOBAL file, ncclAllGather of one file per rank, their union
 * (gys_hll_merge_files_dev) into d_regs[0] / its estimate into d_est[0] (DEVICE; either may be NULL, not both) -- the same on every rank */
int gys_hll_global_rccl(gys_ctx *ctx, void *comm, uint8_t *d_regs, double *d_est);

/* -------------------------------------------------------------------------------------------------------------------
 * a service's response-time t-digest in the external forms of the Postgres tdigest type, so that the reference's SQL
 * percentile aggregation -- public.tdigest(col, 100) / public.tdigest_percentile(digest, p), common/gy_query_common.cc:1818-1855,
 * extension loaded at :3387 -- can consume engine digests ('<text>'::public.tdigest, or the binary send/recv form).
 *   text:   "flags 1 count N compression 100 centroids K (mean, count) ..."     NUL terminated; *needed = strlen
 *   binary: int32 flags, int64 count, int32 compression, int32 ncentroids, K x {float8 mean, int64 count}, network byte order
 * The digest handed over is the merged view (clusters + still buffered values).  GYS_ERR_NOMEM when buflen is too small (*needed
 * is set), GYS_ERR_NOTFOUND for a service without values (the type has no empty literal). */
int gys_tdigest_sql_text(gys_ctx *ctx, uint64_t glob_id, char *buf, size_t buflen, size_t *needed);
int gys_tdigest_sql_binary(gys_ctx *ctx, uint64_t glob_id, void *buf, size_t buflen, size_t *needed);

/* -------------------------------------------------------------------------------------------------------------------
 * multi-level windows (gys_config.enable_levels).  Replaces the per-listener RESP_TIME_HISTOGRAM =
 * TIME_HISTOGRAM<RESP_TIME_HASH, Level_5s_5min_5days_all> (common/gy_statistics.h:1082-1551, :2067), i.e. folly::MultiLevelTimeSeries
 * per histogram bucket with 10 ring buckets per level, and the QPS_HISTOGRAM / ACTIVE_CONN_HISTOGRAM behind LISTENER_DAY_STATS
 * (common/gy_socket_stat.h:548-549).  Every gys_window_prepare(tusec) is one add_histogram_data(tnow = tusec / 10^6, window
 * histogram, flush) of every service (gy_statistics.h:1213-1247); a query at tusec first advances the series to that time
 * (get_stats_with_flush :1369).  Times are whole seconds and must not go backwards (folly clamps, so does the engine).
 * level: 0 = the window closed last ("last 5 seconds": the engine's tumbling window itself; empty once 5 s have passed since its
 * close), 1 = last 300 s, 2 = last 5 days (rings of GYS_LEVEL_RING buckets, so between 9/10 and 10/10 of the nominal span, exactly
 * as folly's rings), 3 = since start.  Only windows closed by gys_window_prepare are in a level, never the open one. */
#define GYS_NLEVELS 4
#define GYS_LEVEL_RING 10 /* ntimeseries_buckets, common/gy_statistics.h:1104 */
typedef struct {
	int64_t data_value;
	float percentile; /* 0..100 */
	uint32_t pad;
} gys_time_hist_val; /* == TIME_HIST_VAL, common/gy_statistics.h:489-498 */
/* TIME_HISTOGRAM::get_stats_with_flush(level, pstats, nstats, tcount, tsum, mean_val, tnow) :1333-1374 */
int gys_query_hist_level_stats(gys_ctx *ctx, uint64_t glob_id, int level, uint64_t tusec, gys_time_hist_val *pstats, uint32_t nstats,
			       int64_t *tcount, int64_t *tsum, double *mean_val);
/* TIME_HISTOGRAM::get_level_data :1166-1200 for a range of services; out[i].max_val_seen = the all-time maximum for every level */
int gys_export_hist_level(gys_ctx *ctx, int level, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out);
/* TIME_HISTOGRAM::get_stats_for_period_with_flush(starttime, endtime, pstats, nstats, tcount, tsum, mean_val, tnow) :1378-1413: the
 * statistics of the seconds [starttime, endtime], answered as folly does -- from the first level whose span reaches back to
 * starttime (tnow - 5 / 300 / 432000 s <= starttime, else since start), its ring buckets weighted by the fraction of each that the
 * interval covers (float, truncated: BucketedTimeSeries::rangeAdjust).  The since-start level is one bucket from the service's
 * first window close to tnow.  tusec = tnow in microseconds.  Level 0 is the engine's tumbling window (see above), so an interval
 * that starts within the last 5 s sees the window closed last or nothing. */
int gys_query_hist_period_stats(gys_ctx *ctx, uint64_t glob_id, int64_t starttime, int64_t endtime, uint64_t tusec, gys_time_hist_val *pstats,
				uint32_t nstats, int64_t *tcount, int64_t *tsum, double *mean_val);
/* the interval's {count, sum} per histogram bucket for a range of services (slabhist.buckets_[b].count(start, end) / sum(start, end));
 * out[i].total_count = their sum, max_val_seen = the all-time maximum; level_used (may be NULL) = the level that answered */
int gys_export_hist_period(gys_ctx *ctx, int64_t starttime, int64_t endtime, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out,
			   int *level_used);

typedef struct {
	uint64_t glob_id;
	int64_t tcount_5d, tsum_5d;
	uint32_t p95_5d_respms, p25_5d_respms, p95_qps, p25_qps, p95_nactive, p25_nactive;
} gys_listener_day_stats; /* == comm::LISTENER_DAY_STATS, 48 bytes, common/gy_comm_proto.h:1620-1632 */
/* What TCP_LISTENER::get_curr_state puts into LISTENER_DAY_STATS (common/gy_socket_stat.cc:2053-2112) for a range of services, as the
 * NOTIFY_LISTENER_DAY_STATS payload madhava consumes (handle_listener_day_stats server/gy_mconnhdlr.cc:12805).  The reference sends
 * zeros for a listener younger than 15 minutes; listener start times are control-plane state, that rule is left to the caller. */
int gys_export_day_stats(gys_ctx *ctx, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_listener_day_stats *out);
/* the per-service QPS (which = 0, SEMI_LOG_HASH_LO) / active-connection (which = 1, HASH_1_3000) histograms fed by listener state */
int gys_export_svc_hist(gys_ctx *ctx, int which, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out);

/* -------------------------------------------------------------------------------------------------------------------
 * the same queries as JSON in the reference's web shapes (field names and order = common/gy_json_field_maps.h):
 *   gys_json_svcsumm      {"madid":..,"summstats":[{time,nidle,ngood,nok,nbad,nsevere,ndown,totqps,totaconn,totkbin,totkbout,totsererr,
 *                          nsvc,nactive}],"hostinfo":{parid,host,madid,cluster}}   MCONN_HANDLER::web_curr_listener_summ (gy_mnodehandle.cc:1628)
 *   gys_json_svcstate     {"madid":..,"svcstate":[{time,svcid,name,qps5s,...,state,issue,ishttp,desc}],"hostinfo":{..}}
 *                          MCONN_HANDLER::web_curr_listener_state (gy_mnodehandle.cc:4650), json_db_svcstate_arr (:1102-1135)
 *   gys_json_clusterstate {"shyamaid":..,"clusterstate":[{time,cluster,nhosts,nprocissue,nprochosts,nproc,nlistissue,nlisthosts,nlisten,
 *                          totqps,svcnetmb,ncpuissue,nmemissue}]}   SHCONN_HANDLER::web_curr_clusterstate (gy_shnodehandle.cc:508)
 * buf receives a NUL-terminated string; *needed = strlen of the full result; GYS_ERR_NOMEM when buflen is too small.
 * timestr: the "time" field as the caller wants it printed (the reference prints local ISO-8601); NULL = "". */
int gys_set_host_name(gys_ctx *ctx, const uint8_t machine_id[16], const char *hostname); /* PARTHA_INFO::hostname_ for "host" */
int gys_json_svcsumm(gys_ctx *ctx, const uint8_t machine_id[16], const char *madhava_id16, const char *timestr, char *buf, size_t buflen, size_t *needed);
int gys_json_svcstate(gys_ctx *ctx, const uint8_t machine_id[16], const char *madhava_id16, const char *timestr, char *buf, size_t buflen, size_t *needed);
int gys_json_clusterstate(gys_ctx *ctx, const char *shyama_id16, const char *timestr, char *buf, size_t buflen, size_t *needed);
/* MCONN_HANDLER::web_curr_top_listeners (server/gy_mnodehandle.cc:2706-3190): {"madid":..,"topissue":[..],"topqps":[..],"topactconn":[..],
 * "topnet":[..],"summstats":{..}[,"hostinfo":{..}]}.  machine_id: one partha's four top-10 queues (+ hostinfo); NULL: every host's queues
 * merged into GYS_MULTI_TOPN = 50 slots per kind (MAX_MULTI_TOPN, common/gy_json_field_maps.h:481), entries carrying parid / host / madid /
 * cluster.  Entry = the svcstate fields + ip (empty: the registry holds (netns, port)) + port.  flags: which arrays to send. */
#define GYS_MULTI_TOPN 50
enum { GYS_TOP_ISSUE = 1, GYS_TOP_QPS = 2, GYS_TOP_ACTCONN = 4, GYS_TOP_NET = 8, GYS_TOP_SUMMSTATS = 16 };
int gys_json_toplisteners(gys_ctx *ctx, const uint8_t machine_id[16], uint32_t flags, const char *madhava_id16, const char *timestr, char *buf,
			  size_t buflen, size_t *needed);

/* ---- QUERY_OPTIONS on the live listener table: multi-host filter / sort / maxrecs and the aggregation operators --------------------------
 * Replaces the listener walk of MCONN_HANDLER::web_curr_listener_state (server/gy_mnodehandle.cc:4650-4900: every MTCP_LISTENER of every
 * partha under RCU, a SvcStateFields per listener, `filter_match` per row, `nrecs >= maxrecs`) for criteria on the numeric columns of
 * json_db_svcstate_arr (common/gy_json_field_maps.h:1102-1135): ONE device pass over the kept state records of all services.
 * Columns (SvcStateFields::get_num_field server/gy_mfields.h:1402-1440; every one is compared as an `int`, `issue` as int16_t; `state` is the
 * numeric OBJ_STATE_E a filter names through statefromjson, `ishttp` 0 / 1): */
enum { GYS_SVC_COL_QPS5S = 0, GYS_SVC_COL_NQRY5S, GYS_SVC_COL_RESP5S, GYS_SVC_COL_P95RESP5S, GYS_SVC_COL_P95RESP5M, GYS_SVC_COL_NCONNS,
       GYS_SVC_COL_NACTIVE, GYS_SVC_COL_NPROCS, GYS_SVC_COL_KBIN15S, GYS_SVC_COL_KBOUT15S, GYS_SVC_COL_SERERR, GYS_SVC_COL_CLIERR,
       GYS_SVC_COL_DELAYUS, GYS_SVC_COL_CPUDELUS, GYS_SVC_COL_IODELUS, GYS_SVC_COL_VMDELUS, GYS_SVC_COL_USERCPU, GYS_SVC_COL_SYSCPU,
       GYS_SVC_COL_RSSMB, GYS_SVC_COL_NISSUE, GYS_SVC_COL_STATE, GYS_SVC_COL_ISSUE, GYS_SVC_COL_ISHTTP, GYS_SVC_NCOLS };
/* comparators: the numeric members of COMPARATORS_E with its numbering (common/gy_query_criteria.h:28-46; match_num_criterian :1243-1290) */
enum { GYS_COMP_EQ = 0, GYS_COMP_NEQ, GYS_COMP_LT, GYS_COMP_LE, GYS_COMP_GT, GYS_COMP_GE, GYS_COMP_BIT2, GYS_COMP_BIT3, GYS_COMP_IN = 12, GYS_COMP_NOTIN = 13 };
#define GYS_SVC_MAX_TERMS 16
#define GYS_SVC_MAX_GROUPS 8
#define GYS_SVC_MAX_AGGR 8
typedef struct {
	uint8_t col;        /* GYS_SVC_COL_* */
	uint8_t comp;       /* GYS_COMP_* */
	uint8_t group;      /* criteria group of the term: 0 = CRITERIA_SET::l1_grp_, 1.. = its L2 groups (< GYS_SVC_MAX_GROUPS) */
	uint8_t reserved;
	uint32_t nvalues;   /* GYS_COMP_IN / NOTIN: the values are set_values[set_first .. set_first + nvalues) of the filter */
	uint32_t set_first;
	uint32_t reserved2;
	int64_t value;      /* the other comparators: converted to the column's own type before the compare, as the reference does */
} gys_svc_term;
typedef struct {
	const gys_svc_term *terms;
	uint32_t nterms;                         /* 0 = no criteria: every current record is listed (CRIT_SKIP) */
	uint32_t nset_values;
	const int64_t *set_values;
	uint8_t group_oper[GYS_SVC_MAX_GROUPS];  /* per group: 0 = all its terms must match (OPER_AND), 1 = any (OPER_OR); match_criteria_group :1535-1605 */
	uint8_t top_oper;                        /* how the groups combine: 0 = AND, 1 = OR (CRITERIA_SET::l1_oper_, match_criteria :1806-1900) */
	uint8_t reserved[3];
	uint32_t nmachine_ids;                   /* 0 = all hosts (is_multihost_); else only the listeners of these parthas ... */
	const uint8_t *machine_ids;              /* ... nmachine_ids x 16 bytes */
	/* criteria on the string columns that select rather than compare (all three AND with each other and with the terms): */
	const uint64_t *svcids;                  /* svcid = / in (...): only these listeners -- the reference's direct-lookup path      */
	uint32_t nsvcids;                        /*   (server/gy_mnodehandle.cc:4754-4860); 0 = not restricted; unknown ids match nothing */
	uint32_t nclusters;                      /* cluster = / in (...): only hosts of these clusters (names as registered); 0 = not restricted */
	const char *const *clusters;
} gys_svc_filter;
typedef struct {
	uint32_t slot, host_slot; /* service slot (gys_lookup_service) and host slot (gys_register_host) */
	uint8_t rec[88];          /* the kept comm::LISTENER_STATE_NOTIFY of the listener */
} gys_svc_row;
/* The records whose state is current (this or the last window: the reference lists states at most 10 s old, :4660) and that pass the
 * filter; at most maxrecs of them, ordered by sort_col (GYS_SVC_COL_*; descending when sort_desc) and then by service slot -- sort_col < 0:
 * by service slot (registration order; the reference's order is that of its hash-table walk).  When more records match than maxrecs the
 * FIRST maxrecs of that order are returned (an exact top-k on the device).  *nmatched = records that matched. */
int gys_query_svcstate_scan(gys_ctx *ctx, const gys_svc_filter *filter, int sort_col, int sort_desc, uint32_t maxrecs, gys_svc_row *out,
			    uint32_t *nout, uint64_t *nmatched);
/* A criterion on the service's NAME (SvcStateFields "name" / "svcname": a string field, server/gy_mfields.h): the glob_ids of the
 * registered services whose process name (gys_listener_info.comm) matches -- to be handed to gys_svc_filter.svcids.  comp = the
 * reference's string comparators with its numbering (COMPARATORS_E common/gy_query_criteria.h:28-45; match_str_criterian :1335-1383):
 * GYS_COMP_EQ / NEQ (whole name), GYS_COMP_SUBSTR / NOTSUBSTR (memmem), GYS_COMP_LIKE / NOTLIKE (a regular expression matched anywhere in
 * the name, as RE2::PartialMatch -- here a linear-time automaton search over bytes (gys_regex.hpp) with RE2's syntax minus its Unicode
 * classes, \\C and \\Q..\\E; never a backtracking search: a pattern from a web query cannot stall the criterion; an invalid or unsupported
 * expression is GYS_ERR_INVAL as the reference's ERR_INVALID_REQUEST), GYS_COMP_IN / NOTIN (any / none of npatterns whole names).  The other comparators use patterns[0].  Host-side:
 * the names never leave the host.  *nout = services that match; GYS_ERR_NOMEM when that exceeds cap (the first cap are written). */
enum { GYS_COMP_SUBSTR = 8, GYS_COMP_NOTSUBSTR = 9, GYS_COMP_LIKE = 10, GYS_COMP_NOTLIKE = 11 };
int gys_svc_ids_by_name(gys_ctx *ctx, int comp, const char *const *patterns, uint32_t npatterns, uint64_t *out_ids, uint32_t cap, uint32_t *nout);
/* ... and on the HOST name (gys_set_host_name: PARTHA_INFO::hostname_, the "host" column): the machine ids of the registered hosts whose
 * name matches, 16 bytes each, for gys_svc_filter.machine_ids (a host without a name has the empty name). */
int gys_machine_ids_by_hostname(gys_ctx *ctx, int comp, const char *const *patterns, uint32_t npatterns, uint8_t *out_ids16, uint32_t cap, uint32_t *nout);
/* the same as the reference's multi-host JSON: {"madid":..,"svcstate":[{"parid","host","madid","cluster", then the json_db_svcstate_arr
 * columns}, ...]} (column list of a multi-host query: QUERY_OPTIONS::get_all_column_list common/gy_query_common.h:418-437) */
int gys_json_svcstate_multihost(gys_ctx *ctx, const gys_svc_filter *filter, int sort_col, int sort_desc, uint32_t maxrecs,
				const char *madhava_id16, const char *timestr, char *buf, size_t buflen, size_t *needed);
/* AGGR_OPER_E (common/gy_json_field_maps.h:114-129) over the records that pass the filter, grouped by nothing (group_by 0: one row,
 * group 0), by host (1: group = host slot) or by cluster (2: group = cluster index in registration order).  One row per group that has a
 * matching record, in group order; every row carries count and, per requested column, the exact 64-bit sum, min and max, from which
 * gys_svc_aggr_value derives the operator: sum, avg (sum / count), max, min, count, bool_or, bool_and.  (percentile: see
 * gys_query_svcstate_percentiles; first / last have no meaning on one snapshot of the live table and are not built.)  *nrows = rows there are (may exceed maxrows; only maxrows are written). */
enum { GYS_AOPER_SUM = 1, GYS_AOPER_AVG, GYS_AOPER_MAX, GYS_AOPER_MIN, GYS_AOPER_COUNT, GYS_AOPER_BOOL_OR = 9, GYS_AOPER_BOOL_AND = 10 };
typedef struct {
	uint32_t group, ncols;
	uint64_t count;
	int64_t sum[GYS_SVC_MAX_AGGR], min[GYS_SVC_MAX_AGGR], max[GYS_SVC_MAX_AGGR];
} gys_svc_aggr_row;
int gys_query_svcstate_aggr(gys_ctx *ctx, const gys_svc_filter *filter, int group_by, const uint8_t *cols, uint32_t ncols, gys_svc_aggr_row *out,
			    uint32_t maxrows, uint32_t *nrows);
int gys_svc_aggr_value(const gys_svc_aggr_row *row, uint32_t col_index, int oper, double *out);
/* AOPER_PERCENTILE (AGGR_OPER_E common/gy_json_field_maps.h:114-129) of ONE column over all records that pass the filter: out[i] = the
 * discrete percentile pcts[i] (0 < p <= 1: the smallest value with at least that fraction of the matching records at or below it, SQL
 * percentile_disc), exact -- the k-th key of the sorted scan found by the same radix selection, nothing gathered.  *nmatched = records
 * that matched (0: out[] is zero).  For a percentile per host or cluster, name the group in the filter (machine_ids / clusters). */
int gys_query_svcstate_percentiles(gys_ctx *ctx, const gys_svc_filter *filter, int col, const double *pcts, uint32_t npcts, int64_t *out, uint64_t *nmatched);
/* The multi-host form of web_curr_listener_summ (server/gy_mnodehandle.cc:1628-1690: the walk over partha_tbl_, SvcSummFields::filter_match per
 * host, hosts whose listener state is older than 10 s skipped): {"madid":..,"summstats":[{"parid","host","madid","cluster", then the
 * json_db_svcsumm_arr columns}, ...]} for every host that reported listener states in the last finished window and passes the filter.  The
 * filter is a gys_svc_filter whose terms name the numeric columns of json_db_svcsumm_arr (common/gy_json_field_maps.h:1396-1416):
 * GYS_SUMM_COL_*; machine_ids / clusters select hosts, svcids is ignored.  Rows in host-slot order, or sorted by sort_col (then host slot);
 * at most maxrecs rows.  (A few thousand 52-byte rows: filtered on the host side after one copy of the per-host summaries.) */
enum { GYS_SUMM_COL_NIDLE = 0, GYS_SUMM_COL_NGOOD, GYS_SUMM_COL_NOK, GYS_SUMM_COL_NBAD, GYS_SUMM_COL_NSEVERE, GYS_SUMM_COL_NDOWN, GYS_SUMM_COL_TOTQPS,
       GYS_SUMM_COL_TOTACONN, GYS_SUMM_COL_TOTKBIN, GYS_SUMM_COL_TOTKBOUT, GYS_SUMM_COL_TOTSERERR, GYS_SUMM_COL_NSVC, GYS_SUMM_COL_NACTIVE, GYS_SUMM_NCOLS };
int gys_json_svcsumm_multihost(gys_ctx *ctx, const gys_svc_filter *filter, int sort_col, int sort_desc, uint32_t maxrecs, const char *madhava_id16,
			       const char *timestr, char *buf, size_t buflen, size_t *needed);

/* -------------------------------------------------------------------------------------------------------------------
 * Roll-up digests and distinct counts of the services a FILTER selects, per GROUP: the WHERE and the GROUP BY of the aggregated percentile
 * the reference computes in Postgres, public.tdigest_percentile(col, 100, p) over a set of listeners' rows
 * (common/gy_query_common.cc:1818-1855) -- "p99 of the services whose state is bad, per cluster", "distinct flows to these 40 svcids",
 * "p95 of the same service across all its hosts" (the aggregation MAGGR_LISTENER / aggr_glob_id_ stands for).  One call: the filter pass,
 * the members of every group gathered on the device, then the roll-up kernels of gys_tdigest_rollup_dev / gys_hll_rollup_dev on them.
 *
 * Labels: a caller-assigned dense group index per service (its own map of aggr_glob_id_ / a service name to 0 .. G-1).  Every service
 * starts at GYS_NO_GROUP.  groups[i] < gys_config.max_services or GYS_NO_GROUP; every id is checked before anything is applied: an unknown
 * id or a group out of range is GYS_ERR_INVAL and changes nothing.  An id named twice keeps the later group. */
#define GYS_NO_GROUP 0xFFFFFFFFu
int gys_set_service_groups(gys_ctx *ctx, const uint64_t *glob_ids, const uint32_t *groups, uint32_t n);

typedef struct {
	uint32_t group, nmembers; /* host slot / cluster index / label / 0; services in it */
} gys_rollup_row;
enum { GYS_GROUP_NONE = 0, GYS_GROUP_HOST = 1, GYS_GROUP_CLUSTER = 2, GYS_GROUP_LABEL = 3 }; /* 0 .. 2 as gys_query_svcstate_aggr */
#define GYS_RF_ANY_STATE 1u
/* MEMBERS.  flags 0: exactly the services gys_query_svcstate_scan lists for `filter` with an unlimited maxrecs -- state record current, the
 * terms pass, machine_ids / svcids / clusters select them.  GYS_RF_ANY_STATE: every registered service is a candidate whatever the age of
 * its state record; the terms are evaluated on the kept record (all zero if the service never reported) and the selections still apply -- the
 * form for a deployment that ingests response events only.
 * GROUP of a member: GYS_GROUP_NONE: 0; _HOST: its host slot; _CLUSTER: its host's cluster index; _LABEL: its label (a service labelled
 * GYS_NO_GROUP is in no group).
 * ROWS (HOST): one per group that has a member, in ascending group order (the rule of gys_query_svcstate_aggr).  *nrows = such groups; it may
 * exceed maxrows, then the first maxrows groups are computed and written.  Row r owns d_slabs[r], file r of d_regs
 * (gys_hll_file_bytes each, 16-byte aligned) and d_est[r] (DEVICE, maxrows entries each).  Any of the three may be NULL, not all:
 * d_slabs needs enable_tdigest, d_regs / d_est need svc_hll_p (GYS_ERR_STATE otherwise).  rows and *nrows are valid on return (one small
 * read of the counts inside the call); the device outputs follow in stream order (gys_sync).
 * SCRATCH: the digests need 64 KB of value bins per COMPUTED row (min(*nrows, maxrows) rows; kept by the context, grown on demand) besides the
 * caller's maxrows slabs / files / estimates: size maxrows by the groups there can be (1, gys_num_hosts, gys_num_clusters, the highest label
 * set + 1), not by the number of services -- 10^4 label groups are 640 MB of bins, 10^7 would be 640 GB.
 * hll_level -1: the open window's registers (as gys_hll_rollup_dev); 0 .. 3: the level's files at tusec (as gys_hll_rollup_level_dev; needs
 * svc_hll_levels, GYS_ERR_STATE otherwise); anything else GYS_ERR_INVAL, as are an unknown group_by, unknown flags and NULL filter / rows /
 * nrows.  (A filter without terms and selections -- all zero -- selects everything.)
 * DEFINITIONS.  A group's digest is the DIRECT union by value bin of its member services (every member's clusters and buffered values
 * into the group's bins, then the cut into clusters) -- not a roll-up of host slabs: a filtered GYS_GROUP_CLUSTER group holding all
 * services of a cluster is the same distribution as, but NOT bit-equal to, the GYS_ROLLUP_CLUSTER slab, which goes through the host
 * slabs; GYS_GROUP_HOST groups holding all services of their hosts ARE bit-equal to GYS_ROLLUP_HOST.  A group's register file is the
 * byte-wise maximum of its members' files (bit-equal to the fixed roll-ups of the same members at every scope), its estimate the one
 * estimator on those bytes.  Both are independent of the order of the members: results are bit-reproducible.
 * No engine state is modified; concurrency as the other query calls.  ACROSS RANKS there is no collective of its own: every rank runs the
 * call with the same filter and labels, the caller all-gathers its rows' slabs / files and joins the rows of one group with
 * gys_tdigest_merge_slabs_dev / gys_hll_merge_files_dev. */
int gys_rollup_filtered_dev(gys_ctx *ctx, const gys_svc_filter *filter, uint32_t flags, int group_by, int hll_level, uint64_t tusec,
			    gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows, gys_tdigest_slab *d_slabs, uint8_t *d_regs, double *d_est);

/* -------------------------------------------------------------------------------------------------------------------
 * Top-k: WHICH services or groups a scan's results name -- "the 100 services with the worst p99", "the 50 with the lowest share inside
 * 200 ms", "the 20 hosts with the most distinct clients" -- without copying a column of one double per service to the host and sorting it
 * there.  Builder-defined.  The definition is FROZEN.  For a DEVICE column d_col of doubles:
 *   1. The value of row r is d_col[r * stride] (stride = doubles between rows, >= 1).
 *   2. The candidate rows are 0 .. nrows - 1 (d_rows NULL), or the nrows DISTINCT row numbers at d_rows (DEVICE), in any order.
 *   3. A candidate r is ELIGIBLE when its value is not a NaN and, if d_weight (DEVICE, indexed by row number) is given, d_weight[r] >= min_weight.
 *   4. Values compare as real numbers: -0.0 equals +0.0, -infinity is below and +infinity above every finite value.
 *   5. GYS_TOPK_LARGEST: larger value first, then the LOWER row number.  GYS_TOPK_SMALLEST: smaller value first, then the lower row number.
 *   6. out (HOST) holds the first min(k, eligible) rows of that total order, in that order: row, value = the column's stored bits (a -0.0
 *      stays a -0.0), weight = d_weight[r], or 0 without d_weight.  *nout = the entries written, *neligible (may be NULL) = the eligible rows.
 * The result is a function of the SET of candidate rows alone: the order of d_rows (for a filter's member list, whatever the device's atomics
 * left) does not change a bit of it.  k == 0 writes nothing and still reports *neligible.  GYS_ERR_INVAL: NULL column or nout, stride 0, an
 * unknown order, k > 0 with out == NULL.  One small read of the counts inside the call, then the entries; no state is modified.
 * Cost is linear in nrows whatever the values: a column of 10^7 equal values is a legal input (the ties are cut by row number on the device).
 * ACROSS RANKS there is no collective of its own: the top-k of the union is the top-k of the ranks' own top-k lists (rows made global by
 * the caller), so every rank runs the call and the k entries per rank are gathered and ordered again.
 * GROUPS need no call of their own -- a roll-up, the slabs' figures, the selection.  "The 20 hosts with the worst p99":
 *     gys_tdigest_rollup_dev(ctx, GYS_ROLLUP_HOST, d_slabs);                                      one slab per host slot
 *     q = 0.99;  gys_tdigest_slab_quantiles_dev(ctx, d_slabs, nhosts, &q, 1, d_p99);              d_p99[host slot]
 *     gys_tdigest_slab_ranks_dev(ctx, d_slabs, nhosts, &x, 1, d_below, d_total);                  d_total[host slot]: hosts without data drop out
 *     gys_topk_dev(ctx, d_p99, 1, nhosts, NULL, d_total, 1, GYS_TOPK_LARGEST, 20, out, &n, NULL); out[i].row = the host slot
 * and likewise on the rows of gys_rollup_filtered_dev (row = the index into its rows[]) and on its d_est array. */
typedef struct {
	uint32_t row, reserved;
	double value;
	uint64_t weight;
} gys_topk_entry; /* 24 bytes */
enum { GYS_TOPK_LARGEST = 0, GYS_TOPK_SMALLEST = 1 };
int gys_topk_dev(gys_ctx *ctx, const double *d_col, uint32_t stride, uint32_t nrows, const uint32_t *d_rows, const uint64_t *d_weight,
		 uint64_t min_weight, int order, uint32_t k, gys_topk_entry *out /* HOST [k] */, uint32_t *nout, uint64_t *neligible);

/* The service ranking in one call: the scan, the filter and the selection.  value is, bit for bit, that service's entry of the scan at the
 * same moment -- for the two rank metrics one division or one subtraction applied to it; total = the digest's total weight as
 * gys_scan_ranks_dev reports it (0 for GYS_TOP_DISTINCT); level and tusec are read by GYS_TOP_DISTINCT only.
 * CANDIDATES: with a filter exactly the members gys_rollup_filtered_dev selects for the same filter and flags (GYS_RF_ANY_STATE or 0) with
 * GYS_GROUP_NONE; filter NULL: every registered slot that is not free.  ELIGIBLE: total >= max(min_total, 1) for the three digest metrics;
 * every candidate for GYS_TOP_DISTINCT (min_total is not used).  Order and ties: "Top-k" above with row = service slot.
 * GYS_ERR_STATE without enable_tdigest (digest metrics), without svc_hll_p (GYS_TOP_DISTINCT) or without svc_hll_levels (a level);
 * GYS_ERR_INVAL for an unknown metric, order, level or flag, NULL nout, k > 0 with out == NULL. */
enum { GYS_TOP_QUANTILE = 0,     /* param = q: the service's gys_scan_quantiles_dev value */
       GYS_TOP_SHARE_WITHIN = 1, /* param = x ms (converted to int64_t): below(x) / (double)total */
       GYS_TOP_MISSES = 2,       /* param = x ms: (double)total - below(x), the responses slower than x */
       GYS_TOP_DISTINCT = 3 };   /* the distinct-flow estimate; level -1 = open window, 0 .. 3 = that level at tusec */
typedef struct {
	uint64_t glob_id;
	uint32_t slot, host_slot;
	double value;
	uint64_t total;
} gys_top_service; /* 32 bytes */
int gys_top_services(gys_ctx *ctx, int metric, double param, int level, uint64_t tusec, const gys_svc_filter *filter /* NULL = every registered service */,
		     uint32_t flags, uint64_t min_total, int order, uint32_t k, gys_top_service *out /* HOST [k] */, uint32_t *nout, uint64_t *neligible);

/* -------------------------------------------------------------------------------------------------------------------
 * Group response-time histograms of the CLOSED windows for the four levels (gys_config.enable_levels; GYS_ERR_STATE when it is 0, and for
 * level 0 when it is 2; level 0 .. 3 as for gys_query_hist_level_stats, GYS_ERR_INVAL otherwise): "p95 / p99 of this host, this cluster,
 * this set of services over the last 5 s / 5 min / 5 days / since the start".  The roll-up digests above are since-start only (a t-digest
 * cannot be subtracted); the exact GY_HISTOGRAM records exist per service at every level, and this is their sum per group.
 *   DEFINITION.  The record of a group at (level, tusec) = GY_HISTOGRAM::add_histogram (common/gy_statistics.h:625-660) of its members'
 *   records exactly as gys_export_hist_level returns them for the same level and tusec: per bucket count += count and sum += sum,
 *   total_count += total_count, max_val_seen = the larger (at every level the all-time maximum, as there).  A group without a member has the
 *   record gys_hist_init_dev leaves: all zero, max_val_seen = INT64_MIN.  Time handling is that of the level records: tq = max(tusec / 10^6,
 *   the last close), never the open window.
 *   PERCENTILES of the group records: gys_hist_percentiles_dev(GYS_RESP_TIME_HASH, d_out, ngroups, ...) -- the reference's get_percentiles
 *   (common/gy_statistics.h:707-791) on the summed record; no percentile code of its own.
 *   BIT-EXACT and order-free: the adds are 64-bit integer adds (they commute and associate mod 2^64) and a maximum, so every path gives the
 *   same bits -- any member order, services -> hosts -> cluster as well as services -> cluster directly, the fixed scopes as well as an
 *   all-selecting filtered call grouped by host or cluster.
 *   No per-service level records are materialised (the members' level views are worked out in registers); scratch kept by the context: one
 *   record per chunk of 1024 members plus one per host.  No engine state a query can see is modified; concurrency as the other query calls;
 *   asynchronous: the device outputs follow in stream order (gys_sync).
 *   ACROSS RANKS there is no collective of its own: every rank runs the call, the caller all-gathers its records and adds the records of one
 *   group with gys_hist_merge_dev. */
/* one record per host slot (gys_num_hosts) / registered cluster (gys_num_clusters) / one, of `level` (0..3) at tusec, into d_out (DEVICE):
 * the sum of the members' records as gys_export_hist_level returns them at the same tusec.  Scopes as gys_tdigest_rollup_dev; works with
 * enable_tdigest = 0 and svc_hll_p = 0 too.  GYS_ERR_INVAL for an unknown scope or level or a NULL d_out */
int gys_hist_rollup_level_dev(gys_ctx *ctx, int scope, int level, uint64_t tusec, gys_hist_rec *d_out);
/* the same for the services a filter selects, per group: members, groups, rows, maxrows / *nrows rules exactly those of
 * gys_rollup_filtered_dev; row r owns d_recs[r] (DEVICE, maxrows records).  Without services, or with a label domain of 0: GYS_OK and
 * *nrows = 0.  GYS_ERR_INVAL for an unknown group_by / flags / level or NULL filter / rows / nrows / d_recs */
int gys_hist_rollup_filtered_dev(gys_ctx *ctx, const gys_svc_filter *filter, uint32_t flags, int group_by, int level, uint64_t tusec,
				 gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows, gys_hist_rec *d_recs);

/* -------------------------------------------------------------------------------------------------------------------
 * Group response-time histograms for ANY PERIOD, group QPS / active-connection histograms, day statistics per group: the per-service
 * questions gys_export_hist_period, gys_export_svc_hist and gys_export_day_stats asked of a host, a cluster, the rank or the rows of a filtered
 * selection.  The roll-up digests are since-start only (a t-digest cannot be subtracted), so the group record of a period IS the windowed
 * percentile of a group: "p95 of this cluster between 14:00 and 14:30" = get_stats_for_period_with_flush asked of a group.
 *   GROUP PERIOD RECORD at (starttime, endtime, tusec) = GY_HISTOGRAM::add_histogram (common/gy_statistics.h:625-660) of the members' records
 *   exactly as gys_export_hist_period returns them for the same three arguments: per bucket b < 15 count and sum are the 64-bit sums of the
 *   members' values -- the scaling and truncation of a partly covered ring bucket (float, BucketedTimeSeries::rangeAdjust) happen per MEMBER and
 *   per RING BUCKET, before the add, the since-start level's per-service bucket [first close, tq + 1) included; the group record is therefore
 *   NOT a function of the group's level records and is computed by a pass over the members on the device.  total_count = the sum of the
 *   members' total_count = the sum of the group's 15 counts; max_val_seen = the largest of the members' all-time maxima; no member: all zero,
 *   max_val_seen = INT64_MIN.  The answering level depends on starttime, tq and enable_levels only: the same for every member, returned once
 *   through level_used (may be NULL; set whether or not there is a group).  Argument rules, tq = max(tusec / 10^6, the last close), "never the
 *   open window" and the enable_levels = 0 (GYS_ERR_STATE) / 2 (no 5-s level: the 300-s ring answers) behaviour are those of
 *   gys_export_hist_period; no interval is rejected there, none is here.
 *   GROUP QPS / ACTIVE-CONNECTION HISTOGRAMS: which = 0 QPS (SEMI_LOG_HASH_LO), 1 active connections (HASH_1_3000); the group record is the same
 *   sum over the members' records as gys_export_svc_hist returns them; no member: all zero with INT64_MIN.  A member that never reported
 *   carries max_val_seen = INT32_MIN, the value gys_create leaves in these per-service records, so a group whose members never reported shows
 *   INT32_MIN, not INT64_MIN.  The definition is this library's: the distribution of the 5-s samples of the group's listeners (the reference
 *   keeps these histograms per listener only).  Percentiles: gys_hist_percentiles_dev with GYS_SEMI_LOG_HASH_LO / GYS_HASH_1_3000.
 *   GROUP DAY STATISTICS: one gys_listener_day_stats per group; glob_id = the group index (host slot, cluster index, 0, the row's group);
 *   tcount_5d / tsum_5d / p95 / p25 from the group's level-2 record at tusec, p95 / p25 of QPS and active connections from the two group
 *   histograms, all by the rule gys_export_day_stats applies to a service's records.  A group without members (a host slot without services,
 *   a cluster without hosts) has glob_id and zeros.
 *   BIT-EXACT and order-free, as the level records above: everything after the per-member rule is 64-bit integer addition and a maximum, so
 *   services -> hosts -> cluster equals services -> cluster directly, and an all-selecting filtered call grouped by host or cluster equals the
 *   fixed scopes.  Scopes, outputs per host slot / cluster / one, rows, maxrows, *nrows, GYS_RF_ANY_STATE, labels and "no services: GYS_OK,
 *   *nrows = 0" are those of gys_hist_rollup_level_dev / gys_hist_rollup_filtered_dev.  Scratch kept by the context (one record per chunk of
 *   1024 members, one per host, three per group for the day statistics); nothing is kept per service.  No engine state a query can see is
 *   modified; asynchronous on the context stream (gys_sync).  GYS_ERR_STATE without enable_levels; GYS_ERR_INVAL for an unknown scope, which,
 *   group_by or flags and for NULL outputs, filter, rows or nrows.
 *   ACROSS RANKS there is no collective of its own: the caller all-gathers the group records and adds the records of one group with
 *   gys_hist_merge_dev, as for the levels (day statistics across ranks: from the merged records). */
int gys_hist_rollup_period_dev(gys_ctx *ctx, int scope, int64_t starttime, int64_t endtime, uint64_t tusec, gys_hist_rec *d_out, int *level_used);
int gys_hist_rollup_period_filtered_dev(gys_ctx *ctx, const gys_svc_filter *filter, uint32_t flags, int group_by, int64_t starttime, int64_t endtime,
					uint64_t tusec, gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows, gys_hist_rec *d_recs, int *level_used);
int gys_svc_hist_rollup_dev(gys_ctx *ctx, int scope, int which, gys_hist_rec *d_out);
int gys_svc_hist_rollup_filtered_dev(gys_ctx *ctx, const gys_svc_filter *filter, uint32_t flags, int group_by, int which, gys_rollup_row *rows,
				     uint32_t maxrows, uint32_t *nrows, gys_hist_rec *d_recs);
int gys_day_stats_rollup_dev(gys_ctx *ctx, int scope, uint64_t tusec, gys_listener_day_stats *d_out);
int gys_day_stats_rollup_filtered_dev(gys_ctx *ctx, const gys_svc_filter *filter, uint32_t flags, int group_by, uint64_t tusec, gys_rollup_row *rows,
				      uint32_t maxrows, uint32_t *nrows, gys_listener_day_stats *d_out);

/* The per-listener 5-second scan from the engine's OWN state (needs gys_config.enable_levels): replaces the loop of
 * TCP_SOCK_HANDLER::listener_stats_update (common/gy_socket_stat.cc:4044-4365) that turns every listener's counters and histograms into
 * one comm::LISTENER_STATE_NOTIFY (common/gy_comm_proto.h:2183-2254), and the data-parallel part of TCP_LISTENER::get_curr_state
 * (:2030-2143): the p95 bucket ids of the 5-s / 5-min / 5-day levels and the QPS / active-connection histogram percentiles it compares.
 * Call it after the window close at `tusec` (level 0 = the window closed last).  One pass over all services, nothing is modified.
 *   d_notify (device, 88 B x gys_num_services, or NULL): LISTENER_STATE_NOTIFY records with glob_id_, nqrys_5s_ (= the 5-s level's count),
 *            total_resp_5sec_, nconns_ / nconns_active_ (CONN_BITMAP::get_conn_breakup maximum, common/gy_socket_stat.h:413-429),
 *            p95_5s_resp_ms_, p95_5min_resp_ms_, curr_state_ (STATE_IDLE when the QPS is 0, else STATE_OK: the state POLICY -- task / cpu /
 *            memory issue inputs, issue strings -- is not the engine's); every other field 0.  They can be handed to
 *            gys_ingest_listener_state_dev as they are (host roll-up, top-N, QPS / active-connection histogram samples).
 *   d_scan   (device, gys_listener_scan x gys_num_services, or NULL).
 *   qps_multiple = TCP_SOCK_HANDLER::get_bpf_qps_multiple(); diffsec = seconds since the previous scan (:4046, :4109). */
typedef struct {
	uint64_t glob_id;
	int64_t tcount[4], tsum[4];                 /* RESP_STATS::tcount_ / tsum_ of the 5 s / 5 min / 5 d / all-time levels */
	int32_t p95_ms[4], p99_ms[4], p25_ms[4];    /* RESP_STATS::stats_[0..2].data_value */
	int32_t last_qps;                           /* total_queries * multiple / diffsec (last_qps_count_) */
	int32_t curr_qps;                           /* max(last_qps, tcount[0] / 5) */
	int32_t qps_p95, qps_p25, act_p95, act_p25; /* GY_HISTOGRAM::get_percentiles {95, 25} of the QPS / active-connection histograms */
	uint8_t b5, b300, b5day;                    /* get_bucketid_from_threshold<RESP_TIME_HASH>(p95 of the level) */
	uint8_t nconn_active;                       /* max over nactive_conn_arr */
	uint8_t nactive_conn_arr[15];               /* CONN_BITMAP::get_conn_breakup of the window closed last */
	uint8_t reserved[5];
} gys_listener_scan;
int gys_scan_listener_state_dev(gys_ctx *ctx, uint64_t tusec, float qps_multiple, uint32_t diffsec, void *d_notify, gys_listener_scan *d_scan);

/* The listener's state decision: TCP_LISTENER::get_curr_state (common/gy_socket_stat.cc:2020-2870) and its caller's part (:4241-4266) for
 * ALL listeners at once -- OBJ_STATE_E / LISTENER_ISSUE_SRC from the scan records above and from the inputs the listener's own histograms do
 * not hold (task status, host CPU / memory issue flags, server errors, connection count, dependent servers), which the reference takes from
 * RELATED_LISTENERS::LISTENER_TASK_STATUS / is_task_issue (:1914, :2043) and from the host's CPU / memory monitors.  Every branch of the
 * reference that is a function of those values is evaluated (the issue STRING is not produced).  The two history bytes of a listener
 * (TCP_LISTENER::issue_bit_hist_, high_resp_bit_hist_: common/gy_socket_stat.h:656-657) are engine state, advanced by every call.
 *   d_scan      (device) gys_listener_scan x gys_num_services, as gys_scan_listener_state_dev left them;
 *   d_issue_in  (device, or NULL = no errors, no task / host issue, ten days of history) gys_listener_issue_in x gys_num_services;
 *   d_notify    (device, or NULL) the 88-byte records of the scan: curr_state_ @79, curr_issue_ @80, issue_bit_hist_ @81, high_resp_bit_hist_ @82
 *               and, from the inputs, ser_errors_ @44, tasks_delay_usec_ @52, tasks_cpudelay_usec_ @56, tasks_blkiodelay_usec_ @60, ntasks_issue_ @76 (nconns_ @16 when inputs are given) are filled in;
 *   d_out       (device, or NULL) gys_listener_decision x gys_num_services. */
enum { GYS_LI_TASK_ISSUE = 1, GYS_LI_SEVERE = 2, GYS_LI_DELAY = 4, GYS_LI_CPU_ISSUE = 8, GYS_LI_MEM_ISSUE = 16, GYS_LI_DEPENDS = 32, GYS_LI_YOUNG = 64 };
typedef struct {
	uint32_t ser_errors;                                                   /* get_curr_state's ser_errors argument */
	uint32_t tasks_delay_msec, tasks_cpudelay_msec, tasks_blkiodelay_msec; /* LISTENER_TASK_STATUS::tasks_*_usec_ / 1000 (:2047, :2784-2785) */
	int32_t nconn;                                                         /* last_chk_nconn_ (:2040) */
	uint16_t ntasks_issue, ntasks_noissue;                                 /* is_task_issue's counts (:2043-2044) */
	uint8_t flags;                                                         /* GYS_LI_*: task_issue, is_severe, is_delay, cpu_issue, mem_issue, dependent servers exist (:2823-2829), started less than 100 s ago (:4244) */
	uint8_t pad[3];
	int64_t tdiff_start;                                                   /* seconds the listener's response histogram covers (:2033-2034); <= 0: the full 5 days */
} gys_listener_issue_in;
typedef struct {
	uint8_t state, issue;                       /* OBJ_STATE_E (0 Idle, 1 Good, 2 OK, 3 Bad, 4 Severe), LISTENER_ISSUE_SRC (common/gy_json_field_maps.h:242-250, :419-434) */
	uint8_t issue_bit_hist, high_resp_bit_hist; /* the listener's history bytes after this call */
	uint16_t decided_line;                      /* the line of common/gy_socket_stat.cc whose `return` (or the function's end, 2866; 4262 = "just started") decided */
	uint16_t pad;
} gys_listener_decision;
int gys_decide_listener_state_dev(gys_ctx *ctx, const gys_listener_scan *d_scan, const gys_listener_issue_in *d_issue_in, void *d_notify,
				  gys_listener_decision *d_out);

/* -------------------------------------------------------------------------------------------------------------------
 * parity / checkpoint exports (host destination buffers) -- GY_HISTOGRAM::get_serialized analogue (gy_statistics.h:665-673) */
uint32_t gys_num_services(gys_ctx *ctx);
uint32_t gys_num_hosts(gys_ctx *ctx);
int gys_lookup_service(gys_ctx *ctx, uint64_t glob_id, uint32_t *slot);
int gys_export_hist(gys_ctx *ctx, int which, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out);
/* CONN_BITMAP rows of the open window: per service 32 u16 rows of resp_bitmap_v4_ followed by the 32 rows of resp_bitmap_v6_ (common/gy_socket_stat.h:645, :665) */
int gys_export_conn_bitmap(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint16_t *out /* [nslots*64] */);
int gys_export_hll(gys_ctx *ctx, uint8_t *out /* [1 << GYS_HLL_P] */);
int gys_export_cms(gys_ctx *ctx, int which, void *out /* which 0: u32[D*W]; which 1: i64[D*W] */);
int gys_export_tdigest(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, int64_t *sums /* [nslots*100] */, uint32_t *cnts /* [nslots*100] */,
		       int32_t *minmax /* [nslots*2] */);
/* values a service's t-digest still buffers unmerged (unordered; only the first npend[i] entries of row i are meaningful) */
int gys_export_tdigest_pending(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint32_t *npend /* [nslots] */,
			       int32_t *pend /* [nslots * gys_td_pend_cap(ctx)] */);
uint32_t gys_td_pend_cap(gys_ctx *ctx); /* the context's td_pend_cap (GYS_TD_PEND_CAP when the configuration left it 0) */
/* per-service connection counters of the TCP_CONN_NOTIFY roll-up, [nslots*4]: nconn, nclose, bytes_sent, bytes_rcvd.  CONNECTIONS, not
 * records: only the ACCEPTING partha's records count (is_tcp_accept_event_, a loopback record included; the connecting half names the
 * same ser_glob_id_ and would count the connection twice), nconn += 1 on a record with notified_before_ clear (the open notification, or
 * the only record of a short-lived connection), nclose += 1 on a record with tusec_close_ set, bytes as reported (server/gy_mconnhdlr.cc:
 * 9129-9181).  gys_query_cms(which 0 / 1) estimates the same nconn / bytes per service for the last finished window. */
int gys_export_svc_counters(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint64_t *out);
int gys_export_pair_cms(gys_ctx *ctx, int which, void *out /* which 0 / 2 / 4: u32[D*W]; which 1 / 3 / 5: i64[D*W]; see gys_query_pair_cms */);
int gys_export_active_conn_counters(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint64_t *out /* [nslots*4]: rows, bytes_sent, bytes_received, active conns */);
int gys_export_global_hist(gys_ctx *ctx, gys_hist_rec *out); /* all-service response histogram of the last finished window (all ranks) */
int gys_export_svc_hll(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint8_t *out /* [nslots << svc_hll_p] */);
/* the same rows for a level of the closed windows at time tusec (gys_config.svc_hll_levels; "distinct-flow counts of the closed windows") */
int gys_export_svc_hll_level(gys_ctx *ctx, int level, uint64_t tusec, uint32_t first_slot, uint32_t nslots, uint8_t *out /* [nslots << svc_hll_p] */);

/* -------------------------------------------------------------------------------------------------------------------
 * Live active-connection rows: "who talks to this service?", "what does this client call?" by enumeration.  The reference answers from
 * activeconntbl / remoteconntbl (rows written by insert_active_conns, server/gy_mconnhdlr.cc:7780-7928; the Active Conn query reads the
 * rows of the last 25 s, server/gy_mnodehandle.cc:3699-3735; fields json_db_activeconn_arr, common/gy_json_field_maps.h:1479-1495).  With
 * gys_config.actconn_pair_cap = N > 0 every row gys_ingest_active_conns[_dev] takes also goes into an exact table on the device
 * (gyeeta_amd/csrc/gys_actpairs.hpp).  Builder-defined, like the Count-Min gauge of gys_query_pair_cms.  The definition is FROZEN.
 *   KEY     (listener_glob_id_, cli_aggr_task_id_, kind): kind 0 = a local-listener row, 1 = an is_remote_listen_ row.  Local rows are stored
 *           whether or not the listener is registered (the reference writes them without a lookup, server/gy_mconnhdlr.cc:7818-7821).  A row
 *           with an id of 0xFFFFFFFFFFFFFFFF (the table's free marker) is not stored: it is counted as rows_bad_key.
 *   ENTRY   the key's report of the LATEST window in which the key was named.  window = that window number; active_conns (u32), bytes_sent,
 *           bytes_received (u64) and nrows are SUMS over all rows of the key in that window, across calls; cli_delay_msec, ser_delay_msec and
 *           max_rtt_msec are MAXIMA (floats compared as non-negative values: a negative or NaN value counts as 0.0f); the flag bits are ORed;
 *           ser_comm, cli_comm, remote_machine_id and remote_madhava_id come from ONE row, whole: the highest-index row of the last call of
 *           that window that named the key.  A report in a newer window REPLACES the figures, it does not add to them.
 *   LIVE    while (open window) - window <= 3: the open window and the three closed before it -- the "last report" rule of
 *           gys_query_pair_cms which 0 / 1; a report is visible at once (in stream order).  Entries that are not live are never reported.
 *   gys_delete_listeners does not touch the table: rows of a listener that is not registered read slot == GYS_NOSLOT and age out.
 *   ROOM    no row is dropped while (live keys) + (the call's new keys) <= actconn_pair_cap: before a call that could fill more than half of
 *           the entries the live entries are re-inserted into the table's second buffer (a small read-back; gys_actconn_tblstats.rebuilds).
 *           Beyond that a row that finds no entry is dropped and counted (rows_dropped), all rows of a key alike.
 * Single rank: the table holds what this context ingested (it is not exchanged at the window boundary).
 * Every call below answers GYS_ERR_STATE when actconn_pair_cap is 0. */
#define GYS_NOSLOT 0xFFFFFFFFu
typedef struct { /* 128 bytes */
	uint64_t listener_glob_id, cli_aggr_task_id;
	char ser_comm[16], cli_comm[16];
	uint8_t remote_machine_id[16];
	uint64_t remote_madhava_id, bytes_sent, bytes_received;
	uint32_t cli_delay_msec, ser_delay_msec;
	float max_rtt_msec;
	uint32_t active_conns, nrows, window;
	uint32_t slot; /* kind 0: the listener's service slot NOW, or GYS_NOSLOT (not registered, deleted); kind 1: GYS_NOSLOT */
	uint8_t flags, kind, pad[2]; /* flags: the ORed flag byte of the rows (bit 0 cli_listener_proc_, bit 1 is_remote_listen_, bit 2 is_remote_cli_) */
	uint64_t reserved;
} gys_actconn_row;
/* which fields of a selection apply; neither KIND flag = both kinds */
enum { GYS_ACS_BY_LISTENER = 1, GYS_ACS_BY_CLIENT = 2, GYS_ACS_BY_HOST = 4, GYS_ACS_KIND_LOCAL = 8, GYS_ACS_KIND_REMOTE = 16 };
typedef struct {
	uint32_t struct_size; /* = sizeof(gys_actconn_sel) */
	uint32_t flags;       /* GYS_ACS_* */
	uint64_t listener_glob_id, cli_aggr_task_id;
	uint64_t min_bytes;   /* bytes_sent + bytes_received >= min_bytes */
	uint32_t host_slot;   /* GYS_ACS_BY_HOST: the LOCAL rows whose listener is registered on that host */
	uint32_t min_active_conns;
} gys_actconn_sel;
/* the live entries the selection matches (sel NULL = all), compacted into the DEVICE array d_out in any order: min(*nmatch, cap) rows are
 * written (d_out may be NULL with cap 0: a count).  One small read of the count inside the call.  GYS_ERR_INVAL: NULL nmatch, a wrong
 * struct_size, unknown flags, cap > 0 without d_out. */
int gys_actconn_list_dev(gys_ctx *ctx, const gys_actconn_sel *sel, gys_actconn_row *d_out, uint32_t cap, uint32_t *nmatch);
/* the same on the HOST, ordered by (listener id, client id, kind) ascending.  *nmatch > cap: GYS_ERR_NOMEM, *nmatch is set, *nout = 0 and
 * nothing else is written. */
int gys_actconn_list(gys_ctx *ctx, const gys_actconn_sel *sel, gys_actconn_row *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch);
/* one row per service slot, d_out[slot * 4 + 0 .. 3] (DEVICE) = {live client groups, active connections, bytes sent + received, rows} over the
 * live LOCAL entries whose listener is registered now: exact integers stored as doubles (accumulated in integers, converted once); free
 * slots and slots without live entries are 0.  Columns for gys_topk_dev ("the 20 services with the most client groups": d_col = d_out,
 * stride 4).  Asynchronous on the context stream. */
int gys_actconn_svc_stats_dev(gys_ctx *ctx, double *d_out /* [gys_num_services * 4] */);
typedef struct {
	uint64_t entries;      /* entries of one buffer: a power of two >= 2 x actconn_pair_cap */
	uint64_t occupied;     /* entries that hold a key, live or not */
	uint64_t live_keys;    /* live entries now */
	uint64_t rows_dropped; /* rows that found no entry */
	uint64_t rows_bad_key; /* rows with the free marker as an id */
	uint64_t rebuilds;     /* times the live entries moved to the other buffer */
} gys_actconn_tblstats;
int gys_actconn_table_stats(gys_ctx *ctx, gys_actconn_tblstats *out);
/* {"madid":..,"activeconn":[{time,svcid,svcname,cprocid,cname,cparid,cmadid,cnetout,cnetin,cdelms,sdelms,rttms,nconns,csvc}]}: the kind-0 rows
 * the selection matches, in the order of gys_actconn_list; field names and order = json_db_activeconn_arr (common/gy_json_field_maps.h:
 * 1479-1495), number formats = the row insert_active_conns prints (server/gy_mconnhdlr.cc:7869-7873: ids as %016lx, cparid = the two
 * halves of remote_machine_id_, rttms with three decimals, csvc = cli_listener_proc_).  Buffer and *needed as for the other gys_json_*
 * calls.  The client side's shape (json_db_clientconn_arr) is not produced: kind-1 rows are reachable through the list calls. */
int gys_json_activeconn(gys_ctx *ctx, const gys_actconn_sel *sel, const char *madhava_id16, const char *timestr, char *buf, size_t buflen,
			size_t *needed);

/* -------------------------------------------------------------------------------------------------------------------
 * Service dependency graph: "what is downstream / upstream of X, within N hops?"  The reference's service flow map joins
 * activeconn.cprocid to svcprocmap (json_db_svcprocmap_arr, common/gy_json_field_maps.h:1626-1633); a listener's process group arrives
 * as NEW_LISTENER::ser_aggr_task_id_ (common/gy_comm_proto.h:1538).  Here the join runs on the device over the live active-connection
 * rows above (gyeeta_amd/csrc/gys_svcdeps.hpp).  Builder-defined.  The definition is FROZEN.
 *   BINDING a registered listener may be bound to ONE task group (gys_set_listener_tasks; 0 = none).  The binding is identity, like the
 *           label: host state, not part of a service record (gys_service_blob_bytes / gys_svc_state_bytes do not move), not carried by
 *           gys_pack_services.  gys_delete_listeners clears it; a slot handed out again starts unbound.
 *   EDGE    for every LIVE entry (listener id L, client id T, kind k) of the row table -- kind 0 and kind 1 alike: a kind-1 row carries
 *           the local client's task group and the remote listener's id -- with L registered NOW as slot v and T != 0: one edge u -> v
 *           ("u calls v") for EVERY registered slot u bound to T.  The edge is keyed (u, v, k) and carries the entry's figures unsplit
 *           (bytes_sent, bytes_received, active_conns, nrows, window, the ORed flag byte: bit 0 cli_listener_proc_ is reported, it gates
 *           nothing); a pair (u, v) with a row of each kind is two edges.  u == v is an edge like any other.
 *   STATS   a live row whose listener is not registered counts as rows_no_listener; a live row whose client id is 0 or is bound to no
 *           registered listener counts as rows_no_client; a row can count as both.  Neither gives an edge.
 *   HOPS    hops[slot] = the least number of edges from any root to the slot along the chosen direction, 0 for a root, GYS_NOSLOT for a
 *           slot that is not reached or free.  Parallel edges and kinds make no difference to a distance.
 * The graph is derived per call from the table, the registry and the bindings as they are at the call: nothing is cached but the
 * task -> services list (rebuilt after a binding, a delete or a registration).  Single rank, like the table.
 * Every call below answers GYS_ERR_STATE when actconn_pair_cap is 0. */
/* glob_ids[i] is bound to aggr_task_ids[i] (0 clears).  Everything is checked before anything changes: an unknown id gives GYS_ERR_INVAL
 * and nothing is changed; an id named twice keeps its later value. */
int gys_set_listener_tasks(gys_ctx *ctx, const uint64_t *glob_ids, const uint64_t *aggr_task_ids, uint32_t n);
typedef struct { /* 64 bytes */
	uint32_t src_slot, dst_slot;
	uint64_t src_glob_id, dst_glob_id, cli_aggr_task_id, bytes_sent, bytes_received;
	uint32_t active_conns, nrows, window;
	uint8_t kind, flags, pad[2];
} gys_svc_edge;
enum { GYS_SES_BY_SRC = 1, GYS_SES_BY_DST = 2 };
typedef struct {
	uint32_t struct_size; /* = sizeof(gys_svc_edge_sel) */
	uint32_t flags;       /* GYS_SES_*; an id that is not registered matches nothing */
	uint64_t src_glob_id, dst_glob_id;
} gys_svc_edge_sel;
/* the edges the selection matches (sel NULL = all), into the DEVICE array d_out in any order: min(*nmatch, cap) rows are written (d_out may
 * be NULL with cap 0: a count).  One small read of the count inside the call.  GYS_ERR_INVAL: NULL nmatch, a wrong struct_size, unknown
 * flags, cap > 0 without d_out.  More than 2^32 - 1 edges: GYS_ERR_NOMEM. */
int gys_svc_edges_dev(gys_ctx *ctx, const gys_svc_edge_sel *sel, gys_svc_edge *d_out, uint32_t cap, uint32_t *nmatch);
/* the same on the HOST, ordered by (src_slot, dst_slot, kind) ascending.  *nmatch > cap: GYS_ERR_NOMEM, *nmatch is set, *nout = 0 and
 * nothing else is written. */
int gys_svc_edges(gys_ctx *ctx, const gys_svc_edge_sel *sel, gys_svc_edge *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch);
typedef struct {
	uint64_t live_rows;        /* live entries of the row table */
	uint64_t rows_no_listener; /* ... whose listener is not registered */
	uint64_t rows_no_client;   /* ... whose client id is 0 or bound to no registered listener */
	uint64_t edges;
	uint64_t bound_services;   /* registered listeners with a binding */
	uint64_t bound_tasks;      /* distinct task groups among them */
} gys_svcgraph_stats_t;
int gys_svcgraph_stats(gys_ctx *ctx, gys_svcgraph_stats_t *out);
enum { GYS_DEP_CALLEES = 1, GYS_DEP_CALLERS = 2, GYS_DEP_BOTH = 3 }; /* follow u -> v / follow edges backwards / either way at every step */
/* d_hops[slot] (DEVICE, gys_num_services words) = HOPS from the services root_ids (HOST array) names; max_hops 0 = no limit, otherwise
 * slots further away stay GYS_NOSLOT.  Unknown root ids are skipped (with no known root nothing is reached); a root named twice counts
 * once.  *nreached = the slots reached, roots included.  One small read per few levels inside the call.  GYS_ERR_INVAL: dir outside
 * 1 .. 3, NULL d_hops, NULL nreached, NULL root_ids with nroots != 0. */
int gys_svc_deps_dev(gys_ctx *ctx, const uint64_t *root_ids, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *d_hops, uint32_t *nreached);
/* the same on the HOST: the reached services' ids and distances ordered by (hops, slot) ascending.  *nreached > cap: GYS_ERR_NOMEM,
 * *nreached is set, *nout = 0 and nothing else is written. */
int gys_svc_deps(gys_ctx *ctx, const uint64_t *root_ids, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint64_t *glob_ids, uint32_t *hops, uint32_t cap,
		 uint32_t *nout, uint32_t *nreached);

/* -------------------------------------------------------------------------------------------------------------------
 * Service components: "which services form one application?" -- the question in front of "what is within N hops of X".  The reference
 * merges service groups that share a related listener into one effective cluster id on the CPU (SHCONN_HANDLER::coalesce_svc_mesh_locked,
 * server/gy_shconnhdlr.cc:4827-4912: a serial two-pass hash walk) and serves it as "svcmeshclust".  Here the weakly connected components
 * of the dependency graph are computed on the device in a fixed number of launches whatever the graph's diameter
 * (gyeeta_amd/csrc/gys_svccomp.hpp: a lock-free union-find over the edge pairs).  Builder-defined.  The definition is FROZEN.
 * The graph is exactly the one "Service dependency graph" above defines, at the moment of the call: the same live rule, registry, bindings.
 *   COMPONENT two registered slots are in one component when a path of edges joins them, each edge taken in either direction.  Kinds
 *             and parallel edges make no difference; an edge u == v joins nothing; a registered slot with no edge to another slot is a
 *             component of its own.
 *   COMP      comp[slot] = the LOWEST slot number in the slot's component (so comp[comp[s]] == comp[s], and a component's root is one of
 *             its members); GYS_NOSLOT for a free slot.  The result is a function of the graph alone: no launch shape and no order of the
 *             device's atomics can change a bit of it.
 *   COUNTS    ncomp = the components (the registered slots with comp[s] == s); nlinked = those with at least two members.
 *   FIGURES   of a component, each summed modulo 2^64: nservices = its members; nrows = the live table entries that give at least one
 *             edge (all edges of such an entry end at the entry's listener slot v; the entry belongs to comp[v]); nedges = the sum of those
 *             entries' edge counts (self edges count); active_conns, bytes_sent, bytes_received = summed ONCE PER ENTRY, not once per
 *             edge: an entry whose client group owns 70 listeners is one flow, not 70.  Rows that give no edge (rows_no_listener,
 *             rows_no_client) belong to no component.
 * Nothing is cached between calls.  Single rank, like the table.  Every call below answers GYS_ERR_STATE when actconn_pair_cap is 0.
 * MEMBERS of the component of service X need no call of their own: they are what gys_svc_deps(X, GYS_DEP_BOTH, 0) reaches.
 * TOP COMPONENTS by a roll-up figure need none either -- the labels, a grouped roll-up, the selection.  "The 20 applications with the
 * worst p99":
 *     gys_label_service_components(ctx, 2, &ngroups);                                              label = component root, linked ones only
 *     gys_rollup_filtered_dev(ctx, &all, GYS_RF_ANY_STATE, GYS_GROUP_LABEL, -1, 0, rows, ngroups, &nrows, d_slabs, NULL, NULL);
 *                                                                                                  one slab per component, rows[r].group = its root slot
 *     q = 0.99;  gys_tdigest_slab_quantiles_dev(ctx, d_slabs, nrows, &q, 1, d_p99);                d_p99[r]
 *     gys_tdigest_slab_ranks_dev(ctx, d_slabs, nrows, &x, 1, d_below, d_total);                    d_total[r]: components without data drop out
 *     gys_topk_dev(ctx, d_p99, 1, nrows, NULL, d_total, 1, GYS_TOPK_LARGEST, 20, out, &n, NULL);   rows[out[i].row].group = the root slot
 * and likewise with d_est ("most distinct clients per application") or the gys_hist_rollup_*_filtered_dev family ("5-minute histogram
 * per application"). */
/* d_comp (DEVICE, gys_num_services words) = COMP of every slot.  ncomp / nlinked may be NULL: the counts cost two more launches, and are
 * computed only when one is asked for.  One small read of the counter words inside the call besides the two of the edge build; the
 * launches and reads of a call do not depend on the graph.  No engine state is modified.  GYS_ERR_INVAL: NULL d_comp.  With no
 * registered service nothing is written and the counts are 0. */
int gys_svc_components_dev(gys_ctx *ctx, uint32_t *d_comp, uint32_t *ncomp, uint32_t *nlinked);
typedef struct { /* 64 bytes */
	uint32_t root_slot, nservices;
	uint64_t root_glob_id, nedges, nrows, active_conns, bytes_sent, bytes_received, reserved /* 0 */;
} gys_svc_component;
/* the components with nservices >= min_services (0 and 1: all) on the HOST, ordered by (nservices descending, root_slot ascending), with
 * their FIGURES.  *nmatch = such components, *ncomp (may be NULL) = all components.  *nmatch > cap: GYS_ERR_NOMEM, *nmatch and *ncomp
 * are set, *nout = 0 and nothing else is written.  No engine state is modified.  GYS_ERR_INVAL: NULL nout or nmatch, cap > 0 without out. */
int gys_svc_components(gys_ctx *ctx, uint32_t min_services, gys_svc_component *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch,
		       uint32_t *ncomp);
/* The components as roll-up groups: the label (gys_set_service_groups, GYS_GROUP_LABEL) of EVERY slot below gys_num_services becomes
 * comp[slot] when its component has >= min_services members and GYS_NO_GROUP otherwise (free slots included) -- the labels are then
 * exactly what gys_set_service_groups would have left for the same assignment, and whatever label a slot carried before is gone.
 * *ngroups (may be NULL) = the labels in use, i.e. the components with >= min_services members.  The label array is allocated and cleared
 * on first use as gys_set_service_groups does; the label domain is raised to at least gys_num_services (a root slot is below max_services:
 * every rule of the labels holds).  The one call of the three that modifies engine state.
 * The labels are a SNAPSHOT: they do not follow the graph.  Rows that expire, new rows and new bindings change the components, not the
 * labels, until the call is made again; a later gys_delete_listeners or registration treats these labels as it treats caller-set ones
 * (a deleted service's label is cleared, a new one starts at GYS_NO_GROUP), so a group may lose the member whose slot names it. */
int gys_label_service_components(gys_ctx *ctx, uint32_t min_services, uint32_t *ngroups);

/* -------------------------------------------------------------------------------------------------------------------
 * Group flow map: "which cluster talks to which cluster, and how many bytes?  Which hosts does this host depend on?  Which applications
 * feed this one?" -- the dependency graph rolled up to the groups every other roll-up of the library answers for.  It is the view the
 * reference's flow dashboards open with, before anyone drills down to a service.  Here it is a keyed aggregation on the device over the
 * edges of the join (gyeeta_amd/csrc/gys_groupflow.hpp).  Builder-defined.  The definition is FROZEN.
 * The graph is exactly the one "Service dependency graph" above defines, at the moment of the call: the same live rule, registry and
 * bindings, and both kinds of row.
 *   GROUP       of a slot: the rule of gys_rollup_filtered_dev.  group_by is GYS_GROUP_HOST (the slot's host slot), _CLUSTER (its host's
 *               cluster index) or _LABEL (its label); the domains are the registered hosts, the clusters, and the label domain (every
 *               label set so far is below it).  A slot whose group is GYS_NO_GROUP is in no group: a slot with no label, and a label at
 *               or above the domain.  GYS_GROUP_NONE is refused with GYS_ERR_INVAL.  If no label was ever set and group_by is _LABEL,
 *               the call returns GYS_OK with zero rows.
 *   GROUP EDGE  (gu, gv) exists when at least one service edge u -> v has group(u) = gu and group(v) = gv, both real groups.  Kinds and
 *               parallel edges fall into the same group edge.  gu == gv is a group edge like any other: intra-group traffic.
 *   FIGURES     of a group edge, all integers, sums modulo 2^64 -- they do not depend on the order of the device's atomics, and every
 *               comparison is exact.  nedges = the service edges that map to it.  nrows = the live table ENTRIES that contribute.
 *               active_conns, bytes_sent, bytes_received = summed ONCE PER ENTRY AND GROUP EDGE: an entry (L, T, k) has one listener slot
 *               v and m caller slots; it adds its figures once to each DISTINCT (group(u), group(v)) among its m edges, not m times (the
 *               rule of the components: "an entry whose client group owns 70 listeners is one flow, not 70" -- a process group with three
 *               listeners on one host is otherwise counted three times in every HOST and CLUSTER map).  last_window = the maximum of the
 *               entries' window.  kinds: bit 0 is set when a kind-0 entry contributes, bit 1 for a kind-1 entry.  flags = the entries'
 *               flag bytes ORed.
 *   STATS       edges = all service edges (gys_svcgraph_stats.edges); edges_no_group = service edges with an end in no group;
 *               group_edges = the distinct (gu, gv) pairs; self_group_edges = those with gu == gv.
 *   GROUP HOPS  hops[g] = the least number of group edges with gu != gv from any root group to g along the chosen direction (GYS_DEP_*);
 *               0 for a root, GYS_NOSLOT for a group that is not reached.  A root group below the domain is at 0 even if it has no
 *               service; a root at or above the domain is skipped.
 * Nothing is cached between calls, nothing is allocated before the first call, no engine state is modified.  A call makes a fixed number
 * of small reads whatever the graph holds (the search: one more per few levels).  Single rank, like the table.  Every call below answers
 * GYS_ERR_STATE when actconn_pair_cap is 0.
 * GYS_GF_LDS_KEYS: the accumulation sums the equal keys of a tile of 256 table entries in an on-chip table of this many distinct
 * (gu, gv) pairs before anything goes to device memory; a tile that yields more pairs sends the rest to device memory directly.  It
 * changes no result. */
#define GYS_GF_LDS_KEYS 512u
typedef struct { /* 64 bytes */
	uint32_t src_group, dst_group;
	uint64_t nedges, nrows, active_conns, bytes_sent, bytes_received;
	uint32_t last_window;
	uint8_t kinds, flags, pad[2];
	uint64_t reserved; /* 0 */
} gys_group_edge;
enum { GYS_GES_BY_SRC = 1, GYS_GES_BY_DST = 2, GYS_GES_NO_SELF = 4 };
typedef struct {
	uint32_t struct_size; /* = sizeof(gys_group_edge_sel) */
	uint32_t flags;       /* GYS_GES_*; a group that does not exist matches nothing; _NO_SELF leaves out the rows with src_group == dst_group */
	uint32_t src_group, dst_group;
} gys_group_edge_sel;
typedef struct {
	uint64_t edges, edges_no_group, group_edges, self_group_edges;
} gys_group_flow_stats;
/* the group edges the selection matches (sel NULL = all), into the DEVICE array d_out in any order: min(*nmatch, cap) rows are written
 * (d_out may be NULL with cap 0: a count).  The selection applies to the rows returned; *stats (may be NULL) always describes the whole
 * map.  GYS_ERR_INVAL: NULL nmatch, group_by outside GYS_GROUP_HOST .. _LABEL, a wrong struct_size, unknown flags, cap > 0 without
 * d_out.  More than 2^32 - 1 service edges or more than 2^30 possible group edges: GYS_ERR_NOMEM. */
int gys_group_edges_dev(gys_ctx *ctx, int group_by, const gys_group_edge_sel *sel, gys_group_edge *d_out, uint32_t cap, uint32_t *nmatch,
			gys_group_flow_stats *stats);
/* the same on the HOST, ordered by (src_group, dst_group) ascending.  *nmatch > cap: GYS_ERR_NOMEM, *nmatch and *stats are set,
 * *nout = 0 and nothing else is written. */
int gys_group_edges(gys_ctx *ctx, int group_by, const gys_group_edge_sel *sel, gys_group_edge *out, uint32_t cap, uint32_t *nout,
		    uint32_t *nmatch, gys_group_flow_stats *stats);
/* d_hops[g] (DEVICE, one word per group of the domain: at most gys_config.max_hosts words for _HOST, max_clusters for _CLUSTER,
 * max_services for _LABEL) = GROUP HOPS from the groups root_groups (HOST array) names; max_hops 0 = no limit, otherwise groups further away stay
 * GYS_NOSLOT.  A root named twice counts once.  *ndomain (may be NULL) = the words written, *nreached = the groups reached, roots
 * included.  GYS_ERR_INVAL: dir outside 1 .. 3, NULL d_hops, NULL nreached, NULL root_groups with nroots != 0, a bad group_by. */
int gys_group_deps_dev(gys_ctx *ctx, int group_by, const uint32_t *root_groups, uint32_t nroots, uint32_t dir, uint32_t max_hops,
		       uint32_t *d_hops, uint32_t *ndomain, uint32_t *nreached);
/* the same on the HOST: the reached groups and their distances ordered by (hops, group) ascending.  *nreached > cap: GYS_ERR_NOMEM,
 * *nreached is set, *nout = 0 and nothing else is written. */
int gys_group_deps(gys_ctx *ctx, int group_by, const uint32_t *root_groups, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *groups,
		   uint32_t *hops, uint32_t cap, uint32_t *nout, uint32_t *nreached);

/* -------------------------------------------------------------------------------------------------------------------
 * Issue resolution: "400 services are red -- which 5 are the cause, and what did each one take down?"  One of the issue sources
 * gys_decide_listener_state_dev returns is ISSUE_DEPENDENT_SERVER_LISTENER (= 7, common/gy_json_field_maps.h:419-434): "I am slow because
 * something I call is slow".  The reference resolves those every 5 s inside MCONN_HANDLER::partha_listener_state: a listener that is Bad
 * or worse with any OTHER issue is a source (server/gy_mconnhdlr.cc:11325-11349); from it handle_dependency_issue (:10866-10990) walks
 * the listeners of the process groups that depend on it, recursing through those that are Bad with the dependent-listener issue, or OK
 * (:10946-10947), for at most MM_LISTENER_ISSUE_RESOL::MAX_DOWNSTREAM_TIERS = 8 tiers (common/gy_comm_proto.h:2588-2660), and records
 * the source, the tier and the neighbour the issue came through (LISTENER_ISSUE_RESOL, server/gy_msocket.h:28-35) -- a serial recursive
 * hash walk per source.  Here it is a labelled multi-source search on the device over the edge pairs of the join
 * (gyeeta_amd/csrc/gys_svcresol.hpp).  Builder-defined.  The definition is FROZEN.
 * The graph is exactly the one "Service dependency graph" above defines, at the moment of the call: the same live rule, registry and
 * bindings, both kinds of row, single rank.
 * NAMING.  An issue travels from a callee v to its callers u: along the edges u -> v BACKWARDS, the GYS_DEP_CALLERS direction.  In this
 * library a callee is downstream of its caller; the reference's words are the other way round (it calls the source "upstream" and the
 * affected listeners its "downstreams").
 *   STATE     of a slot: (state, issue) = bytes 79 and 80 (curr_state_, curr_issue_) of the slot's kept 88-byte LISTENER_STATE_NOTIFY
 *             record, when that record is CURRENT -- the rule of the service queries: it was kept in the open window or the one before,
 *             it is not marked deleted (a LISTEN_FLAG_DELETE record), and it names this slot's id and host.  With d_dec (a device array
 *             of gys_listener_decision x gys_num_services, as gys_decide_listener_state_dev leaves it) (state, issue) = d_dec[slot].state
 *             and .issue for every REGISTERED slot instead, whatever is kept.  A free slot, a slot without a current record and a
 *             state above 5 have NO STATE.
 *   CLASS     SOURCE: state >= 3 (Bad, Severe, Down) and issue != 7.  DEPENDENT: state >= 3 and issue == 7.  CARRIER: state == 2 (OK).
 *             Everything else is OPAQUE (Idle, Good, no state).  Only DEPENDENT and CARRIER slots take an issue on and pass it further;
 *             a SOURCE or OPAQUE slot on a path blocks it, and a SOURCE is never attributed to another source.
 *   TIER      tier 0 = the SOURCE slots, each its own source.  A DEPENDENT or CARRIER slot u that is not yet attributed gets tier t + 1
 *             when some edge u -> v exists with v attributed at tier t.  Tiers go up to max_tiers: 0 means GYS_RESOL_MAX_TIERS, 1 .. 8 are
 *             taken as given.  Self edges, parallel edges and kinds make no difference.
 *   TIE       among all candidates (source of v, v) at u's tier the lowest source slot wins, then the lowest v.  The result is a function
 *             of the graph and the states alone: no launch shape and no order of the device's atomics can change a bit of it.
 *   ROLE      GYS_RS_NONE (0): OPAQUE, or a CARRIER that was not reached;  GYS_RS_SOURCE (1);  GYS_RS_RESOLVED (2): a DEPENDENT that was
 *             reached;  GYS_RS_CARRIER (3): a CARRIER that was reached;  GYS_RS_UNRESOLVED (4): a DEPENDENT not reached within max_tiers.
 *   RECORD    per slot, gys_svc_resol: src_slot / via_slot = the source and the callee the issue came through, GYS_NOSLOT where there
 *             is none (a source: src_slot = itself, via_slot = GYS_NOSLOT); tier = 0 for every role but RESOLVED and CARRIER; state and
 *             issue as above, 0 where the slot has no state; nresolved = for a SOURCE the RESOLVED slots attributed to it (its blast
 *             radius: carriers are not counted), otherwise 0.
 *   STATS     with_state = the slots with a state; sources, resolved, unresolved, carriers = the slots of that role; edges = all service
 *             edges (gys_svcgraph_stats.edges); resolved_at_tier[t - 1] = the RESOLVED slots at tier t.
 * A call runs a FIXED list of launches -- seed, two per tier (a pass over the pairs, a pass over the slots), finish -- and reads the
 * counter words once behind them, besides the two reads of the edge build: no read inside the search, no "changed" word.  Nothing is
 * cached between calls, nothing is allocated before the first call, no engine state is modified.  Every call below answers
 * GYS_ERR_STATE when actconn_pair_cap is 0.  Not here: attribution across ranks, the reference's 2-s memory of a previous resolution
 * (:11352-11371; a call resolves the states as they are) and its per-related-group any_state_ok_bad_ shortcut.
 * TOP SOURCES need no call of their own.  "The 10 root causes with the most affected services":
 *     gys_svc_resolve_issues_dev(ctx, NULL, 0, d_out, d_impact, NULL);                       d_impact[slot] = nresolved of a source, NaN elsewhere
 *     gys_topk_dev(ctx, d_impact, 1, gys_num_services(ctx), NULL, NULL, 0, GYS_TOPK_LARGEST, 10, out, &n, NULL);   out[i].row = the source's slot */
#define GYS_RESOL_MAX_TIERS 8u
enum { GYS_RS_NONE = 0, GYS_RS_SOURCE = 1, GYS_RS_RESOLVED = 2, GYS_RS_CARRIER = 3, GYS_RS_UNRESOLVED = 4 };
typedef struct { /* 16 bytes */
	uint32_t src_slot, via_slot;
	uint8_t role, tier, state, issue;
	uint32_t nresolved;
} gys_svc_resol;
typedef struct {
	uint64_t with_state, sources, resolved, unresolved, carriers, edges, resolved_at_tier[8];
} gys_svc_resol_stats;
/* d_out[slot] (DEVICE, gys_num_services records, 16-byte aligned: a record leaves in one store) = RECORD of every slot.
 * d_impact (DEVICE, gys_num_services doubles, or NULL): (double)nresolved for a SOURCE and NaN for every other slot -- a column
 * gys_topk_dev takes as it is (it leaves NaNs out).  *stats (HOST, may be NULL).  GYS_ERR_INVAL: NULL or misaligned d_out,
 * max_tiers > 8.  With no registered service nothing is written and the stats are 0. */
int gys_svc_resolve_issues_dev(gys_ctx *ctx, const gys_listener_decision *d_dec /* DEVICE or NULL = kept states */, uint32_t max_tiers,
			       gys_svc_resol *d_out, double *d_impact, gys_svc_resol_stats *stats);
typedef struct { /* 48 bytes */
	uint64_t glob_id, src_glob_id, via_glob_id; /* 0 where there is none */
	uint32_t slot, src_slot, via_slot, nresolved;
	uint8_t role, tier, state, issue, src_state, src_issue, pad[2];
} gys_svc_resol_row;
/* the slots whose role is in role_mask (bit r = list role r; 0 = roles 1 .. 4) on the HOST, ordered by slot ascending; d_dec is a DEVICE
 * array as above.  *nmatch > cap: GYS_ERR_NOMEM, *nmatch and *stats are set, *nout = 0 and nothing else is written.  GYS_ERR_INVAL: NULL
 * nout or nmatch, cap > 0 without out, max_tiers > 8, role bits above 4. */
int gys_svc_resolve_issues(gys_ctx *ctx, const gys_listener_decision *d_dec, uint32_t max_tiers, uint32_t role_mask, gys_svc_resol_row *out,
			   uint32_t cap, uint32_t *nout, uint32_t *nmatch, gys_svc_resol_stats *stats);

/* -------------------------------------------------------------------------------------------------------------------
 * service records: saving, restoring and moving per-service state.  The reference's durable copy of a listener's statistics is Postgres;
 * after a restart the 5-day statistics are re-seeded (handle_listener_req, server/gy_mconnhdlr.cc:14257) through
 * GY_HISTOGRAM::get_serialized / update_from_serialized (common/gy_statistics.h:641-673).  Here the state lives in device memory: the
 * calls below copy it out and back in.  Builder-defined.  The definition is FROZEN.
 *
 * A SERVICE RECORD is the service's part of every per-service array of the context, byte for byte (nothing is folded or normalised
 * first), keyed by glob_id, not by slot.  Its arrays, in record order -- first those whose size is a multiple of 16 bytes:
 *     open-window histogram record (256), all-time record (256), CONN_BITMAP rows (the bitmap line, 128), connection counters (32),
 *     kept listener state (96), active-connection counters (32), per-service HLL file (1 << svc_hll_p; svc_hll_p != 0), the 22
 *     closed-window HLL files (svc_hll_levels: last, 2 x 10 ring, all), with enable_levels: the 2 x 10 level snapshots (256 each), the
 *     level-0 record (256; enable_levels == 1), the QPS and the active-connection histogram (256 each); with enable_tdigest: cluster
 *     sums (200 x 8), cluster counts (200 x 4), the 16-byte buffer bookkeeping (npend, nh, nw, win_epoch, hw_epoch);
 *   then the others, each rounded up to 4 bytes:
 *     connection window accumulators (24), with enable_levels the level-0 tag (4; enable_levels == 1 with enable_tdigest) and the
 *     first-close time (8); with enable_tdigest min / max (8), the buffer cursor (4), the value count of the last batch (4), the
 *     window's response event count (4); the two history bytes of gys_decide_listener_state_dev (2, in a 4-byte word);
 *   zeroes up to a multiple of 16; with enable_tdigest the service's buffered values: td_pend_cap 4-byte words, of which the first
 *     `cursor` are the buffer's (the words behind the cursor are never read, are not carried and are zero in the record), padded to 16.
 * hist_win and the level-0 array change places at every close: the record carries the logical arrays.  NOT in a record: the glob id, the
 * host and the label of a slot (they belong to the destination's registration and to gys_set_service_groups) and what lives within one
 * ingest call (run cursors, the claim word of the state records): the unpack leaves the former alone and sets the latter to their initial
 * values.  The unpack REWRITES one word: the host slot behind the kept 88-byte state (word 23 of the 96-byte entry) becomes the
 * destination's host slot of the service, in every entry that was ever kept (non-zero id words).  No other word of a record names a slot
 * or a host slot.
 *
 * A BLOB is one pack call's output, little-endian, a persistent format:
 *     offset  0  u32 magic 0x42535947 ("GYSB")      4  u32 layout version (1)
 *             8  u32 enable_tdigest (0 / 1)         12  u32 td_pend_cap (the effective value; 0 without t-digest)
 *            16  u32 svc_hll_p                      20  u32 svc_hll_levels (0 / 1)
 *            24  u32 enable_levels                  28  u16 GYS_TD_NB, 30 u16 GYS_LEVEL_RING
 *            32  u32 bitmap line bytes              36  u32 stride: bytes per record, a multiple of 16
 *            40  u32 epoch: the source's open window number
 *            44  u32 n: records
 *            48  i64 lvl_t_last, 56 i64 hl_t_last: the source's last close time (s) of the level rings / of the HLL rings, -1: none
 *            64  n x u64 glob_id, zero-padded to a multiple of 16 bytes
 *            then n records of `stride` bytes in the order of the ids.
 * Offsets 8 .. 39 are the configuration fingerprint that decides the record layout.  max_services, max_hosts, td_buf_values, slot
 * numbers and host slots are not part of a blob: source and destination may differ in all of them.  A blob carries no checksum: its
 * integrity between pack and unpack is the caller's.
 *
 * CLOCK RULE.  Window numbers inside a record (the buffer bookkeeping, word 22 of the kept state, the level-0 tag) and the ring
 * arithmetic of the levels mean something only relative to the context's window number and close times.  Words are never translated:
 *   - a destination that has neither prepared nor closed a window since gys_create (and has not adopted before) ADOPTS the header's epoch,
 *     lvl_t_last and hl_t_last -- the restore case; its first close then clears exactly the ring buckets whose start was crossed since
 *     the source's last close, as an uninterrupted engine would.  What it ingested before the unpack under its own window numbers is
 *     stale afterwards: restore first;
 *   - any other destination must already have the same three values, else GYS_ERR_STATE and nothing is written -- the migration case:
 *     ranks of one job close in lockstep and count alike.
 *
 * gys_pack_services*: modifies no state.  GYS_ERR_INVAL for an unknown or repeated id, a buffer below gys_service_blob_bytes(ctx, n) or a
 * device buffer that is not 16-byte aligned; n = 0 writes a valid empty blob.
 * gys_unpack_services*: OVERWRITES (never merges) the state of every service of the blob whose glob_id is registered in the destination;
 * the other ids are skipped and counted in *nskipped (*napplied, *nskipped may be NULL).  The whole blob is validated before the first
 * store: bad magic, bad version, blob_bytes != what n and stride need, a glob_id that occurs twice: GYS_ERR_INVAL; a fingerprint mismatch
 * (gys_last_error names the field) or the clock rule: GYS_ERR_STATE.  Nothing is modified in any of these cases.
 * Both go through the submission queues' flush first, run on the context stream and return when the device work is done; between
 * gys_window_prepare and gys_window_finish they give GYS_ERR_STATE.  The host-pointer forms move the records through the context's
 * staging buffer in pieces of 8 MB.
 * Only per-service state moves.  The rank-level registers of the open window stay with the source (global HLL, Count-Min tables, host
 * summaries, top-N: all at most three windows old), so move a service RIGHT AFTER a close. */
uint64_t gys_service_blob_bytes(gys_ctx *ctx, uint32_t n); /* header + ids + n records in this context's configuration */
int gys_pack_services_dev(gys_ctx *ctx, const uint64_t *glob_ids /* HOST */, uint32_t n, void *d_blob, uint64_t blob_bytes);
int gys_unpack_services_dev(gys_ctx *ctx, const void *d_blob, uint64_t blob_bytes, uint32_t *napplied, uint32_t *nskipped);
int gys_pack_services(gys_ctx *ctx, const uint64_t *glob_ids, uint32_t n, void *blob /* HOST */, uint64_t blob_bytes);
int gys_unpack_services(gys_ctx *ctx, const void *blob /* HOST */, uint64_t blob_bytes, uint32_t *napplied, uint32_t *nskipped);
/* the glob ids of the registered (not free) slots of [first_slot, first_slot + nslots), in slot order: a checkpoint walks the context in
 * ranges (glob_ids holds nslots entries; the range is cut at gys_num_services) */
int gys_list_service_ids(gys_ctx *ctx, uint32_t first_slot, uint32_t nslots, uint64_t *glob_ids, uint32_t *nout);
/* the glob ids of one host's listeners in slot order (what a partha's move to another rank packs): *nfound = all of them and may exceed
 * cap, the first `cap` are written */
int gys_list_host_service_ids(gys_ctx *ctx, const uint8_t machine_id[16], uint64_t *glob_ids, uint32_t cap, uint32_t *nfound);

typedef struct {
	uint64_t resp_events, resp_dropped_range, resp_dropped_nolistener;
	uint64_t conn_events, conn_unknown_service;
	uint64_t lstate_records, lstate_missed, lstate_errors, lstate_deleted;
	uint64_t resp_batches_host_local, resp_batches_general; /* which resp pipeline each ingest call took (gys_config.resp_path) */
	uint64_t window_graph_launches; /* window boundaries replayed from the captured hipGraph (0: plain stream operations were used) */
	uint64_t resp_batches_host_split; /* host-local pipeline in its split form (few hosts, long segments: parts of 65536 events) */
	uint64_t td_merges, td_merge_values; /* t-digest re-clusterings queued so far and the buffered values they merged */
	uint64_t actconn_records, actconn_remote_listen, actconn_unknown_listener; /* ACTIVE_CONN_STATS rows of local listeners / of listeners on
										      another madhava (is_remote_listen_) / of local listeners not registered */
	uint64_t stage_waits;       /* host-pointer calls that found their staging slot still in flight and waited for the GPU (ring wrapped) */
	uint64_t resp_calls_queued; /* gys_ingest_resp_events calls that went through the submission queue ... */
	uint64_t resp_submissions;  /* ... and the combined batches they were submitted as (calls / submissions = calls per launch set) */
	/* the tallies MCONN_HANDLER::partha_tcp_conn_info keeps while it walks a message (server/gy_mconnhdlr.cc:9133-9137, :9327: nnew,
	 * nclosed, nclosed_no_not), summed over all messages: open notifications / records with tusec_close_ / closes of connections
	 * whose open was never notified.  conn_new + conn_closed_no_notify = connection HALVES seen (each connection is reported by its
	 * accepting and by its connecting partha); conn_client_side = records of the connecting half only (is_tcp_connect_event_ without
	 * is_tcp_accept_event_), which do not enter the per-service counters (see gys_export_svc_counters). */
	uint64_t conn_new, conn_closed, conn_closed_no_notify, conn_client_side;
	uint64_t resp_tail_flushes; /* submissions made by the queue's flusher thread: the tail of a burst of gys_ingest_resp_events calls that
				     * found the GPU busy is submitted ~200 us after a submission retires, without waiting for the next call */
	/* gys_ingest_tcp_conn / gys_ingest_listener_state calls that went through their submission queues, the combined batches they were
	 * submitted as, and the submissions made by those queues' flusher threads */
	uint64_t conn_calls_queued, conn_submissions, lstate_calls_queued, lstate_submissions, rec_tail_flushes;
	uint64_t resp_run_overflow; /* response values a batch could not place (a run past the end of the batch staging area): 0 by construction, checked in the kernel */
} gys_counters;
int gys_get_counters(gys_ctx *ctx, gys_counters *out);
/* response events the submission queue of gys_ingest_resp_events still holds on the HOST side (copied out of the callers' buffers, not yet
 * submitted to the GPU).  Unlike every other entry point this one does not flush the queue: it is the way to watch it drain. */
int gys_resp_queue_pending(gys_ctx *ctx, uint64_t *events);

/* -------------------------------------------------------------------------------------------------------------------
 * standalone keyed histogram op (rows a1/a2/a4 of SURVEY 8a for ANY hash kind): nkeys histograms of `kind`, caller-owned DEVICE
 * memory hist[nkeys] (zero-initialised except max_val_seen = type min, see gys_hist_init_dev). */
int gys_hist_init_dev(gys_ctx *ctx, int kind, gys_hist_rec *d_hist, uint32_t nkeys);
int gys_hist_add_dev(gys_ctx *ctx, int kind, gys_hist_rec *d_hist, uint32_t nkeys, const uint32_t *d_keyidx, const int32_t *d_vals, uint64_t n);
int gys_hist_merge_dev(gys_ctx *ctx, gys_hist_rec *d_dst, const gys_hist_rec *d_src, uint32_t nkeys); /* add_histogram :625 */
int gys_hist_percentiles_dev(gys_ctx *ctx, int kind, const gys_hist_rec *d_hist, uint32_t nkeys, const float *pcts, uint32_t npct,
			     int64_t *d_out);

/* -------------------------------------------------------------------------------------------------------------------
 * measurement helpers: per-kernel HIP-event timing on the context stream */
int gys_profile_enable(gys_ctx *ctx, int on);
int gys_profile_reset(gys_ctx *ctx);
/* name: "resp_host", "key_pass", "digest_merge", "digest_huge" (general pipeline: "resp_pass1", "scan", "scatter"), "conn", "lstate", "wire_decode", ...; returns accumulated ms + launches */
int gys_profile_get(gys_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);
int gys_profile_names(gys_ctx *ctx, char *buf, size_t buflen); /* comma separated */

/* synthetic stream generators running ON the GPU (bench/test plumbing).  They write into caller DEVICE buffers. */
/* zipf_milli: 0 = services uniform; s*1000 = Zipf(s) over the services of a host; GYS_GEN_SPREAD = service weights spread evenly
 * over 0..255/256 (bench.py uses one such pass before timing so that the keys' t-digest buffers start at evenly spread fill levels
 * -- with identical rates and identical start all keys would otherwise overflow in the same window) */
#define GYS_GEN_SPREAD 0xFFFFFFFFu
/* PMC calibration helper: reads nevents 24-byte events with the access pattern of the event kernel (3 x 8-B loads per thread at a 24-B
 * stride) and does nothing else -- FETCH_SIZE of this launch vs the known 24 B x nevents (tools/calibrate_fetch.py) */
int gys_debug_read_events_dev(gys_ctx *ctx, const void *d_ev24, uint64_t nevents);
/* test witness of the large-key t-digest path (keys that bring more than 16 384 values in one call): waits for the work queued so far and
 * copies the path's list lengths.  out[0] large keys of the last response batch, out[1] of them handed to the one-workgroup fallback
 * (both counted over the whole batch); out[2] pool entries, out[3] values >= 16 384 ms put on the tail list (counts on past its
 * capacity), out[4] entries the 512-value merge tier handed to the 16 384-value tier -- these three of the batch's LAST pool round
 * only (an entry the second tier hands on to the fallback is in out[4] and in out[1]).  out[0..2] are cleared at the start of every
 * response batch; out[3] and out[4] are reset by the path's planning kernel, so they keep their values over batches too small to
 * hold a large key.  out[5..7] = 0.  Read-only. */
int gys_debug_huge_counts(gys_ctx *ctx, uint32_t out[8]);
int gys_gen_resp_events_dev(gys_ctx *ctx, void *d_ev24, uint64_t nevents, uint64_t seed, uint32_t first_host, uint32_t nhosts,
			    uint32_t svcs_per_host, uint32_t zipf_milli /* 0 = uniform, else s*1000 */, gys_resp_seg *segs_out /* host, nhosts */);

#ifdef __cplusplus
}
#endif
#endif
