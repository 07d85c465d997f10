"""Host-side wrapper around the C ABI (plumbing for tests / bench).  It mirrors the reference's aggregation entry points
(MCONN_HANDLER::partha_tcp_conn_info / partha_listener_state / send_cluster_state, server/gy_mconnhdlr.h:2091-2156) by name and
argument meaning; the multi-GPU step (one exchange per window) is an all-reduce of the fixed-size sketch registers
through torch.distributed (backend "nccl" == RCCL over xGMI on ROCm; "gloo" in the CPU tests)."""
import ctypes as C
import os

import numpy as np

from . import capi, wire

_TORCH_DTYPES = None


def _torch_dtypes():
    global _TORCH_DTYPES
    if _TORCH_DTYPES is None:
        import torch
        _TORCH_DTYPES = {0: torch.uint8, 1: torch.int32, 2: torch.int64}  # u32 sums wrap identically as int32
    return _TORCH_DTYPES


def allreduce_sections(sections, group=None):
    """sections: list of (tensor, op) with op 0 = MAX, 1 = SUM.  One collective per register family (HLL = max on u8,
    CMS / histogram / cluster counters = sum); no-op when torch.distributed is not initialised or world_size == 1."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    for t, op in sections:
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 0 else dist.ReduceOp.SUM, group=group)


def mid_buf(machine_id):
    assert len(machine_id) == 16
    return (C.c_uint8 * 16)(*machine_id)


class SketchEngine:
    def __init__(self, max_hosts, max_services, max_clusters=16, enable_tdigest=True, svc_hll_p=0, max_batch_events=1 << 20,
                 rank=0, nranks=1, device=None, torch_arena=True, resp_path=0, enable_levels=False, td_buf_values=0, conn_pair_cms=False, td_pend_cap=0,
                 svc_hll_levels=0, actconn_pair_cap=0):
        import torch
        self.L = capi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("SketchEngine needs a HIP device: the sketch engine has no CPU path")
        self.torch = torch
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device)
        cfg = capi.Config()
        cfg.struct_size = C.sizeof(capi.Config)
        cfg.device = int(device)
        cfg.rank, cfg.nranks = rank, nranks
        cfg.max_hosts, cfg.max_services, cfg.max_clusters = max_hosts, max_services, max_clusters
        cfg.enable_tdigest = 1 if enable_tdigest else 0
        cfg.svc_hll_p = svc_hll_p
        cfg.svc_hll_levels = int(svc_hll_levels)  # the registers of the closed windows for the four levels (needs svc_hll_p)
        cfg.actconn_pair_cap = int(actconn_pair_cap)  # live (listener, client task group) rows: room for that many keys (0 = off)
        cfg.resp_path = resp_path
        cfg.enable_levels = int(enable_levels)  # False / True / 2 (without the 5-s level)
        cfg.td_buf_values = td_buf_values
        cfg.td_pend_cap = td_pend_cap
        cfg.conn_pair_cms = 1 if conn_pair_cms else 0
        cfg.max_batch_events = max_batch_events
        with torch.cuda.device(self.device):
            # the engine gets its own torch stream: torch work (tensor fills / copies on the current stream, collectives) and engine work are
            # ordered explicitly -- order() before handing device buffers to the engine, sync() (or stream.synchronize) before reading results
            self.stream = torch.cuda.Stream(device=self.device)
            cfg.stream = self.stream.cuda_stream
            self.arena = None
            if torch_arena:
                nbytes = self.L.gys_reduce_arena_bytes(C.byref(cfg))
                self.arena = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
                cfg.reduce_arena = self.arena.data_ptr()
                cfg.reduce_arena_bytes = nbytes
            h = C.c_void_p()
            capi.check(self.L.gys_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.cfg = cfg
        self.rank, self.nranks = rank, nranks
        self._sections = None

    def order(self):
        """engine work submitted after this call starts after everything queued so far on torch's current stream (e.g. the fill / copy
        that produced a device buffer about to be handed to the engine)"""
        self.stream.wait_stream(self.torch.cuda.current_stream(self.device))

    def close(self):
        if self.h:
            self.L.gys_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- registration
    def register_cluster(self, name):
        idx = C.c_uint32()
        capi.check(self.L.gys_register_cluster(self.h, name.encode(), C.byref(idx)))
        return idx.value

    def register_host(self, machine_id, cluster="cluster0"):
        slot = C.c_uint32()
        capi.check(self.L.gys_register_host(self.h, mid_buf(machine_id), cluster.encode(), C.byref(slot)))
        return slot.value

    def owns(self, machine_id):
        return self.L.gys_shard_of(mid_buf(machine_id), self.nranks) == self.rank

    def _listener_infos(self, glob_ids, netns, ports, comm=b"svc", addrs=None):
        """the gys_listener_info array of a registration call; addrs: per listener None (an any-address listener: NEW_LISTENER::is_any_ip_) or the
        4 / 16 address bytes it is bound to"""
        n = len(glob_ids)
        arr = (capi.ListenerInfo * n)()
        for i in range(n):
            arr[i].glob_id = int(glob_ids[i])
            arr[i].netns = int(netns[i])
            arr[i].port = int(ports[i])
            arr[i].comm = comm
            a = addrs[i] if addrs is not None else None
            arr[i].is_any_ip = 1 if a is None else 0
            if a is not None:
                a = bytes(a)
                arr[i].addr_is_v6 = 1 if len(a) == 16 else 0
                arr[i].addr = (C.c_uint8 * 16)(*(a + bytes(16))[:16])
        return arr

    def register_listeners(self, machine_id, glob_ids, netns, ports, comm=b"svc", addrs=None):
        """addrs: per listener None (an any-address listener: NEW_LISTENER::is_any_ip_) or the 4 / 16 address bytes it is bound to"""
        arr = self._listener_infos(glob_ids, netns, ports, comm, addrs)
        first = C.c_uint32()
        capi.check(self.L.gys_register_listeners(self.h, mid_buf(machine_id), arr, len(glob_ids), C.byref(first)))
        return first.value

    def register_listeners_slots(self, machine_id, glob_ids, netns, ports, comm=b"svc", addrs=None):
        """gys_register_listeners_slots: new ids take the free slots gys_delete_listeners left (lowest first), then the tail; returns the
        slot of every listener (numpy u32), new or known"""
        n = len(glob_ids)
        arr = self._listener_infos(glob_ids, netns, ports, comm, addrs)
        slots = np.zeros(max(n, 1), dtype=np.uint32)
        capi.check(self.L.gys_register_listeners_slots(self.h, mid_buf(machine_id), arr, n, slots.ctypes.data_as(C.POINTER(C.c_uint32))))
        return slots[:n]

    def delete_listeners(self, glob_ids):
        """gys_delete_listeners: the services leave the engine and their slots become free; returns how many were known"""
        ids = np.ascontiguousarray(glob_ids, dtype=np.uint64)
        nd = C.c_uint32()
        capi.check(self.L.gys_delete_listeners(self.h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), len(ids), C.byref(nd)))
        return nd.value

    def num_free_slots(self):
        return self.L.gys_num_free_slots(self.h)

    def svc_state_bytes(self):
        """gys_svc_state_bytes: bytes of per-service device state a delete resets per slot"""
        return self.L.gys_svc_state_bytes(self.h)

    STALE_DELETED, STALE_AGED = 1, 2

    def list_stale_listeners(self, flags=3, max_age_windows=360, cap=1 << 16):
        """gys_list_stale_listeners: (ids of the first `cap` hits in slot order, number of hits)"""
        ids = np.zeros(max(cap, 1), dtype=np.uint64)
        nf = C.c_uint32()
        capi.check(self.L.gys_list_stale_listeners(self.h, flags, max_age_windows, ids.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(nf)))
        return ids[:min(cap, nf.value)].copy(), nf.value

    # ---------------------------------------------------------------- service records ("service records" in gysketch.h)
    def list_service_ids(self, first=0, n=None):
        """gys_list_service_ids: glob ids of the registered (not free) slots of [first, first + n) in slot order (numpy u64)"""
        n = self.num_services() - first if n is None else n
        ids, nout = np.zeros(max(n, 1), dtype=np.uint64), C.c_uint32()
        capi.check(self.L.gys_list_service_ids(self.h, first, max(n, 0), ids.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(nout)))
        return ids[:nout.value].copy()

    def service_blob_bytes(self, n):
        return self.L.gys_service_blob_bytes(self.h, n)

    def pack_services(self, glob_ids=None, dev=False):
        """gys_pack_services / _dev: the blob of the listed services (None: every registered one) as numpy uint8 -- dev: as a torch uint8
        tensor on the device.  Modifies nothing."""
        ids = self.list_service_ids() if glob_ids is None else np.ascontiguousarray(glob_ids, dtype=np.uint64)
        nb = self.service_blob_bytes(len(ids))
        idp = ids.ctypes.data_as(C.POINTER(C.c_uint64))
        if dev:
            blob = self.torch.empty(nb, dtype=self.torch.uint8, device=self.device)
            self.order()
            capi.check(self.L.gys_pack_services_dev(self.h, idp, len(ids), C.c_void_p(blob.data_ptr()), nb))
            return blob
        blob = np.empty(nb, dtype=np.uint8)
        capi.check(self.L.gys_pack_services(self.h, idp, len(ids), C.c_void_p(blob.ctypes.data), nb))
        return blob

    def unpack_services(self, blob):
        """gys_unpack_services / _dev (a torch tensor on the device takes the device form; anything else is host bytes): overwrites the state
        of the blob's services that are registered here; returns (applied, skipped)"""
        na, ns = C.c_uint32(), C.c_uint32()
        if hasattr(blob, "data_ptr"):
            self.order()
            capi.check(self.L.gys_unpack_services_dev(self.h, C.c_void_p(blob.data_ptr()), blob.numel() * blob.element_size(), C.byref(na), C.byref(ns)))
        else:
            b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob).view(np.uint8)
            capi.check(self.L.gys_unpack_services(self.h, C.c_void_p(b.ctypes.data), b.nbytes, C.byref(na), C.byref(ns)))
        return na.value, ns.value

    STATE_FILE_PIECE = 64 << 20

    def save_state(self, path):
        """every registered service to a file: blobs of at most 64 MB over ranges of slots, each behind its length as a little-endian u64
        (the format of the shim's save_all).  Returns the number of services written."""
        per = max(1, (self.STATE_FILE_PIECE - 64) // (self.service_blob_bytes(1) - 64))
        total = 0
        tmp = path + ".tmp"  # written beside the target and renamed over it when complete: a failed save leaves the previous file as it was
        try:
            with open(tmp, "wb") as f:
                for first in range(0, self.num_services(), per):
                    ids = self.list_service_ids(first, per)
                    if len(ids):
                        blob = self.pack_services(ids)
                        f.write(np.uint64(blob.nbytes).tobytes())
                        f.write(blob.tobytes())
                        total += len(ids)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise
        return total

    def load_state(self, path):
        """the blobs of save_state / save_all into the services registered here: (applied, skipped)"""
        applied = skipped = 0
        with open(path, "rb") as f:
            while True:
                head = f.read(8)
                if not head:
                    break
                nb = int(np.frombuffer(head, dtype="<u8")[0]) if len(head) == 8 else -1
                blob = f.read(nb) if nb >= 0 else b""
                if nb < 64 or len(blob) != nb:
                    raise capi.GysError(capi.ERR_INVAL, "truncated state file %s" % path)
                a, s = self.unpack_services(blob)
                applied, skipped = applied + a, skipped + s
        return applied, skipped

    LISTENER_INFO_DT = np.dtype([("glob_id", "<u8"), ("netns", "<u4"), ("port", "<u2"), ("is_any_ip", "u1"), ("addr_is_v6", "u1"), ("comm", "S16"),
                                 ("addr", "u1", (16,))])

    def register_listeners_np(self, machine_id, glob_ids, netns, ports):
        """bulk variant: fills the gys_listener_info array through numpy (no per-element python loop); any-address listeners"""
        n = len(glob_ids)
        a = np.zeros(n, dtype=self.LISTENER_INFO_DT)
        a["glob_id"], a["netns"], a["port"], a["comm"], a["is_any_ip"] = glob_ids, netns, ports, b"svc", 1
        first = C.c_uint32()
        capi.check(self.L.gys_register_listeners(self.h, mid_buf(machine_id), a.ctypes.data_as(C.POINTER(capi.ListenerInfo)), n, C.byref(first)))
        return first.value

    # ---------------------------------------------------------------- ingest (names follow the reference entry points)
    def handle_resp_events(self, machine_id, events):
        """TCP_SOCK_HANDLER::handle_ipv4_resp_event for a host batch (numpy RESP_EVENT array or bytes)"""
        b = events.tobytes() if hasattr(events, "tobytes") else bytes(events)
        capi.check(self.L.gys_ingest_resp_events(self.h, mid_buf(machine_id), b, len(b) // 24))

    def handle_resp_events_v6(self, machine_id, events):
        """TCP_SOCK_HANDLER::handle_ipv6_resp_event for a host batch (numpy RESP_EVENT6 array or bytes)"""
        b = events.tobytes() if hasattr(events, "tobytes") else bytes(events)
        capi.check(self.L.gys_ingest_resp_events_v6(self.h, mid_buf(machine_id), b, len(b) // 48))

    def handle_resp_events_v6_dev(self, segs, d_ev, nevents):
        self.order()
        capi.check(self.L.gys_ingest_resp_events_v6_dev(self.h, segs, len(segs), C.c_void_p(d_ev), nevents))

    def handle_resp_events_dev(self, segs, d_ev, nevents):
        self.order()
        capi.check(self.L.gys_ingest_resp_events_dev(self.h, segs, len(segs), C.c_void_p(d_ev), nevents))

    def partha_tcp_conn_info(self, machine_id, batch_bytes, nconns):
        """MCONN_HANDLER::partha_tcp_conn_info(partha, pone, nconns, pendptr)"""
        buf = np.frombuffer(batch_bytes, dtype=np.uint8)
        buf = np.require(buf, requirements=["A", "C"])
        p = buf.ctypes.data
        capi.check(self.L.gys_ingest_tcp_conn(self.h, mid_buf(machine_id), C.c_void_p(p), nconns, C.c_void_p(p + len(buf))))

    def partha_listener_state(self, machine_id, batch_bytes, nrecs):
        """MCONN_HANDLER::partha_listener_state(partha, pone, nconns, pendptr)"""
        buf = np.frombuffer(batch_bytes, dtype=np.uint8)
        buf = np.require(buf, requirements=["A", "C"])
        p = buf.ctypes.data
        capi.check(self.L.gys_ingest_listener_state(self.h, mid_buf(machine_id), C.c_void_p(p), nrecs, C.c_void_p(p + len(buf))))

    def handle_partha_active_conns(self, machine_id, batch_bytes, nitems):
        """MCONN_HANDLER::handle_partha_active_conns(partha, pconn, nitems, pendptr)"""
        buf = np.frombuffer(batch_bytes, dtype=np.uint8)
        buf = np.require(buf, requirements=["A", "C"])
        p = buf.ctypes.data
        capi.check(self.L.gys_ingest_active_conns(self.h, mid_buf(machine_id), C.c_void_p(p), nitems, C.c_void_p(p + len(buf))))

    def pair_cms(self, listener_glob_id, cli_aggr_task_id, which=0):
        out = C.c_uint64()
        capi.check(self.L.gys_query_pair_cms(self.h, int(listener_glob_id), int(cli_aggr_task_id), which, C.byref(out)))
        return out.value

    def export_pair_cms(self, which=0):
        out = np.zeros((capi.CMS_D, capi.CMS_W), dtype=np.int64 if which & 1 else np.uint32)
        capi.check(self.L.gys_export_pair_cms(self.h, which, C.c_void_p(out.ctypes.data)))
        return out

    def export_active_conn_counters(self, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        capi.check(self.L.gys_export_active_conn_counters(self.h, first, n, out.ctypes.data_as(capi.u64p)))
        return out

    # ---------------------------------------------------------------- live (listener, client task group) rows (actconn_pair_cap)
    ACTCONN_ROW_DT = np.dtype([("listener_glob_id", "<u8"), ("cli_aggr_task_id", "<u8"), ("ser_comm", "S16"), ("cli_comm", "S16"),
                               ("remote_machine_id", "<u8", 2), ("remote_madhava_id", "<u8"), ("bytes_sent", "<u8"), ("bytes_received", "<u8"),
                               ("cli_delay_msec", "<u4"), ("ser_delay_msec", "<u4"), ("max_rtt_msec", "<f4"), ("active_conns", "<u4"), ("nrows", "<u4"),
                               ("window", "<u4"), ("slot", "<u4"), ("flags", "u1"), ("kind", "u1"), ("pad", "u1", 2), ("reserved", "<u8")])

    @staticmethod
    def actconn_sel(listener=None, client=None, host_slot=None, kind=None, min_bytes=0, min_active_conns=0):
        """a gys_actconn_sel: listener / client = the ids to match, host_slot = the local rows of that host's listeners, kind = 0 (local) /
        1 (remote-listener rows) / None (both)"""
        s = capi.ActconnSel()
        s.struct_size = C.sizeof(capi.ActconnSel)
        if listener is not None:
            s.flags |= capi.ACS_BY_LISTENER
            s.listener_glob_id = int(listener)
        if client is not None:
            s.flags |= capi.ACS_BY_CLIENT
            s.cli_aggr_task_id = int(client)
        if host_slot is not None:
            s.flags |= capi.ACS_BY_HOST
            s.host_slot = int(host_slot)
        if kind is not None:
            s.flags |= capi.ACS_KIND_REMOTE if kind else capi.ACS_KIND_LOCAL
        s.min_bytes, s.min_active_conns = int(min_bytes), int(min_active_conns)
        return s

    def actconn_list(self, sel=None, cap=None):
        """gys_actconn_list -> (rc, rows as a numpy ACTCONN_ROW_DT array in (listener, client, kind) order, number of matches); rc is
        capi.ERR_NOMEM (and the array empty) when more rows match than cap.  cap None = the table's entries"""
        if cap is None:
            cap = self.actconn_table_stats()["entries"]
        out = (capi.ActconnRow * max(cap, 1))()
        nout, nmatch = C.c_uint32(), C.c_uint32()
        rc = self.L.gys_actconn_list(self.h, C.byref(sel) if sel is not None else None, out, cap, C.byref(nout), C.byref(nmatch))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, np.frombuffer(out, dtype=self.ACTCONN_ROW_DT, count=nout.value).copy(), nmatch.value

    def actconn_list_dev(self, sel=None, cap=0):
        """gys_actconn_list_dev -> (torch uint8 device tensor of cap rows of 128 bytes, the first min(matches, cap) written; number of matches)"""
        out = self.torch.zeros((max(cap, 1), 128), dtype=self.torch.uint8, device=self.device)
        nmatch = C.c_uint32()
        self.order()
        capi.check(self.L.gys_actconn_list_dev(self.h, C.byref(sel) if sel is not None else None, C.c_void_p(out.data_ptr()), cap, C.byref(nmatch)))
        return out, nmatch.value

    def actconn_svc_stats_dev(self):
        """gys_actconn_svc_stats_dev -> torch float64 device tensor [num_services, 4]: live client groups, active connections, bytes, rows"""
        out = self.torch.zeros((max(self.num_services(), 1), 4), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_actconn_svc_stats_dev(self.h, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def actconn_table_stats(self):
        st = capi.ActconnTblStats()
        capi.check(self.L.gys_actconn_table_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in capi.ActconnTblStats._fields_}

    def json_activeconn(self, sel=None, madid="0" * 16, timestr=""):
        return self._json(self.L.gys_json_activeconn, C.byref(sel) if sel is not None else None, madid.encode(), timestr.encode())

    # ---------------------------------------------------------------- service dependency graph (actconn_pair_cap; "Service dependency graph")
    SVC_EDGE_DT = np.dtype([("src_slot", "<u4"), ("dst_slot", "<u4"), ("src_glob_id", "<u8"), ("dst_glob_id", "<u8"), ("cli_aggr_task_id", "<u8"),
                            ("bytes_sent", "<u8"), ("bytes_received", "<u8"), ("active_conns", "<u4"), ("nrows", "<u4"), ("window", "<u4"),
                            ("kind", "u1"), ("flags", "u1"), ("pad", "u1", 2)])

    def set_listener_tasks(self, glob_ids, aggr_task_ids):
        """gys_set_listener_tasks -> rc (capi.OK, or capi.ERR_INVAL for an unknown id: nothing was changed); task id 0 clears a binding"""
        g = np.ascontiguousarray(glob_ids, dtype=np.uint64)
        t = np.ascontiguousarray(aggr_task_ids, dtype=np.uint64)
        assert len(g) == len(t)
        rc = self.L.gys_set_listener_tasks(self.h, g.ctypes.data_as(capi.u64p), t.ctypes.data_as(capi.u64p), len(g))
        if rc not in (capi.OK, capi.ERR_INVAL):
            capi.check(rc)
        return rc

    @staticmethod
    def svc_edge_sel(src=None, dst=None):
        """a gys_svc_edge_sel: src / dst = the glob_id of the calling / the called service"""
        s = capi.SvcEdgeSel()
        s.struct_size = C.sizeof(capi.SvcEdgeSel)
        if src is not None:
            s.flags |= capi.SES_BY_SRC
            s.src_glob_id = int(src)
        if dst is not None:
            s.flags |= capi.SES_BY_DST
            s.dst_glob_id = int(dst)
        return s

    def svc_edges(self, sel=None, cap=None):
        """gys_svc_edges -> (rc, edges as a numpy SVC_EDGE_DT array in (src_slot, dst_slot, kind) order, number of matches); rc is
        capi.ERR_NOMEM (and the array empty) when more edges match than cap.  cap None = as many as match"""
        ref = C.byref(sel) if sel is not None else None
        if cap is None:
            cap = self.svc_edges_dev(sel, 0)[1]
        out = (capi.SvcEdge * max(cap, 1))()
        nout, nmatch = C.c_uint32(), C.c_uint32()
        rc = self.L.gys_svc_edges(self.h, ref, out, cap, C.byref(nout), C.byref(nmatch))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, np.frombuffer(out, dtype=self.SVC_EDGE_DT, count=nout.value).copy(), nmatch.value

    def svc_edges_dev(self, sel=None, cap=0):
        """gys_svc_edges_dev -> (torch uint8 device tensor of cap rows of 64 bytes, the first min(matches, cap) written; number of matches)"""
        out = self.torch.zeros((max(cap, 1), 64), dtype=self.torch.uint8, device=self.device)
        nmatch = C.c_uint32()
        self.order()
        capi.check(self.L.gys_svc_edges_dev(self.h, C.byref(sel) if sel is not None else None, C.c_void_p(out.data_ptr()), cap, C.byref(nmatch)))
        return out, nmatch.value

    def svcgraph_stats(self):
        st = capi.SvcGraphStats()
        capi.check(self.L.gys_svcgraph_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in capi.SvcGraphStats._fields_}

    def svc_deps_dev(self, roots, direction=capi.DEP_CALLEES, max_hops=0):
        """gys_svc_deps_dev -> (torch int32 device tensor [num_services]: hops per slot, -1 (GYS_NOSLOT) where not reached; services reached)"""
        r = np.ascontiguousarray(roots, dtype=np.uint64)
        out = self.torch.zeros(max(self.num_services(), 1), dtype=self.torch.int32, device=self.device)
        n = C.c_uint32()
        self.order()
        capi.check(self.L.gys_svc_deps_dev(self.h, r.ctypes.data_as(capi.u64p), len(r), direction, max_hops, C.c_void_p(out.data_ptr()), C.byref(n)))
        return out, n.value

    def svc_deps(self, roots, direction=capi.DEP_CALLEES, max_hops=0, cap=None):
        """gys_svc_deps -> (rc, glob_ids, hops, services reached) ordered by (hops, slot); rc is capi.ERR_NOMEM (and the arrays empty) when
        more services are reached than cap.  cap None = num_services"""
        r = np.ascontiguousarray(roots, dtype=np.uint64)
        if cap is None:
            cap = self.num_services()
        ids, hops = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32)
        nout, n = C.c_uint32(), C.c_uint32()
        rc = self.L.gys_svc_deps(self.h, r.ctypes.data_as(capi.u64p), len(r), direction, max_hops, ids.ctypes.data_as(capi.u64p),
                                 hops.ctypes.data_as(capi.u32p), cap, C.byref(nout), C.byref(n))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, ids[:nout.value].copy(), hops[:nout.value].copy(), n.value

    # ---------------------------------------------------------------- service components (actconn_pair_cap; "Service components")
    SVC_COMPONENT_DT = np.dtype([("root_slot", "<u4"), ("nservices", "<u4"), ("root_glob_id", "<u8"), ("nedges", "<u8"), ("nrows", "<u8"),
                                 ("active_conns", "<u8"), ("bytes_sent", "<u8"), ("bytes_received", "<u8"), ("reserved", "<u8")])

    def svc_components_dev(self, counts=True):
        """gys_svc_components_dev -> (torch int32 device tensor [num_services]: the lowest slot of the slot's component, -1 (GYS_NOSLOT) for a
        free slot; components; components with two members or more).  counts=False skips the two counting launches: (tensor, None, None)"""
        out = self.torch.zeros(max(self.num_services(), 1), dtype=self.torch.int32, device=self.device)
        nc, nl = C.c_uint32(), C.c_uint32()
        self.order()
        capi.check(self.L.gys_svc_components_dev(self.h, C.c_void_p(out.data_ptr()), C.byref(nc) if counts else None, C.byref(nl) if counts else None))
        return (out, nc.value, nl.value) if counts else (out, None, None)

    def svc_components(self, min_services=0, cap=None):
        """gys_svc_components -> (rc, components as a numpy SVC_COMPONENT_DT array ordered by (nservices descending, root_slot), matching
        components, all components); rc is capi.ERR_NOMEM (and the array empty) when more match than cap.  cap None = num_services"""
        if cap is None:
            cap = self.num_services()
        out = (capi.SvcComponent * max(cap, 1))()
        nout, nmatch, ncomp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.L.gys_svc_components(self.h, min_services, out, cap, C.byref(nout), C.byref(nmatch), C.byref(ncomp))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, np.frombuffer(out, dtype=self.SVC_COMPONENT_DT, count=nout.value).copy(), nmatch.value, ncomp.value

    def label_service_components(self, min_services=2):
        """gys_label_service_components -> the labels in use: every service's label (GYS_GROUP_LABEL) becomes the root slot of its component
        where that has >= min_services members, GYS_NO_GROUP elsewhere.  A snapshot: the labels do not follow the graph"""
        n = C.c_uint32()
        capi.check(self.L.gys_label_service_components(self.h, min_services, C.byref(n)))
        self._label_domain = max(getattr(self, "_label_domain", 0), self.num_services())  # (a root slot is a label: see set_service_groups)
        return n.value

    # ---------------------------------------------------------------- group flow map (actconn_pair_cap; "Group flow map")
    GROUP_EDGE_DT = np.dtype([("src_group", "<u4"), ("dst_group", "<u4"), ("nedges", "<u8"), ("nrows", "<u8"), ("active_conns", "<u8"),
                              ("bytes_sent", "<u8"), ("bytes_received", "<u8"), ("last_window", "<u4"), ("kinds", "u1"), ("flags", "u1"),
                              ("pad", "u1", 2), ("reserved", "<u8")])

    @staticmethod
    def group_edge_sel(src=None, dst=None, no_self=False):
        """a gys_group_edge_sel: src / dst = the calling / the called group; no_self leaves out the rows with src_group == dst_group"""
        s = capi.GroupEdgeSel()
        s.struct_size = C.sizeof(capi.GroupEdgeSel)
        if src is not None:
            s.flags |= capi.GES_BY_SRC
            s.src_group = int(src)
        if dst is not None:
            s.flags |= capi.GES_BY_DST
            s.dst_group = int(dst)
        if no_self:
            s.flags |= capi.GES_NO_SELF
        return s

    def group_edges_dev(self, group_by, sel=None, cap=0):
        """gys_group_edges_dev -> (torch uint8 device tensor of cap rows of 64 bytes, the first min(matches, cap) written in any order;
        number of matches; the gys_group_flow_stats of the whole map as a dict)"""
        out = self.torch.zeros((max(cap, 1), 64), dtype=self.torch.uint8, device=self.device)
        nmatch, st = C.c_uint32(), capi.GroupFlowStats()
        self.order()
        capi.check(self.L.gys_group_edges_dev(self.h, group_by, C.byref(sel) if sel is not None else None, C.c_void_p(out.data_ptr()), cap, C.byref(nmatch),
                                              C.byref(st)))
        return out, nmatch.value, {k: getattr(st, k) for k, _ in capi.GroupFlowStats._fields_}

    def group_edges(self, group_by, sel=None, cap=None):
        """gys_group_edges -> (rc, group edges as a numpy GROUP_EDGE_DT array in (src_group, dst_group) order, number of matches, stats);
        rc is capi.ERR_NOMEM (and the array empty) when more match than cap.  cap None = as many as match"""
        ref = C.byref(sel) if sel is not None else None
        if cap is None:
            cap = self.group_edges_dev(group_by, sel, 0)[1]
        out = (capi.GroupEdge * max(cap, 1))()
        nout, nmatch, st = C.c_uint32(), C.c_uint32(), capi.GroupFlowStats()
        rc = self.L.gys_group_edges(self.h, group_by, ref, out, cap, C.byref(nout), C.byref(nmatch), C.byref(st))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, np.frombuffer(out, dtype=self.GROUP_EDGE_DT, count=nout.value).copy(), nmatch.value, {k: getattr(st, k) for k, _ in capi.GroupFlowStats._fields_}

    def _group_domain_cap(self, group_by):
        cfg = self.cfg
        return max(int(cfg.max_services if group_by == capi.GROUP_LABEL else cfg.max_clusters if group_by == capi.GROUP_CLUSTER else cfg.max_hosts), 1)

    def group_deps_dev(self, group_by, roots, direction=capi.DEP_CALLEES, max_hops=0):
        """gys_group_deps_dev -> (torch int32 device tensor [domain]: hops per group, -1 (GYS_NOSLOT) where not reached; groups reached)"""
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        out = self.torch.zeros(self._group_domain_cap(group_by), dtype=self.torch.int32, device=self.device)
        nd, n = C.c_uint32(), C.c_uint32()
        self.order()
        capi.check(self.L.gys_group_deps_dev(self.h, group_by, r.ctypes.data_as(capi.u32p), len(r), direction, max_hops, C.c_void_p(out.data_ptr()), C.byref(nd),
                                             C.byref(n)))
        return out[:nd.value], n.value

    def group_deps(self, group_by, roots, direction=capi.DEP_CALLEES, max_hops=0, cap=None):
        """gys_group_deps -> (rc, groups, hops, groups reached) ordered by (hops, group); rc is capi.ERR_NOMEM (and the arrays empty) when
        more groups are reached than cap.  cap None = the largest domain the grouping can have"""
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        if cap is None:
            cap = self._group_domain_cap(group_by)
        groups, hops = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
        nout, n = C.c_uint32(), C.c_uint32()
        rc = self.L.gys_group_deps(self.h, group_by, r.ctypes.data_as(capi.u32p), len(r), direction, max_hops, groups.ctypes.data_as(capi.u32p),
                                   hops.ctypes.data_as(capi.u32p), cap, C.byref(nout), C.byref(n))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, groups[:nout.value].copy(), hops[:nout.value].copy(), n.value

    # ---------------------------------------------------------------- issue resolution (actconn_pair_cap; "Issue resolution")
    SVC_RESOL_DT = np.dtype([("src_slot", "<u4"), ("via_slot", "<u4"), ("role", "u1"), ("tier", "u1"), ("state", "u1"), ("issue", "u1"), ("nresolved", "<u4")])
    SVC_RESOL_ROW_DT = np.dtype([("glob_id", "<u8"), ("src_glob_id", "<u8"), ("via_glob_id", "<u8"), ("slot", "<u4"), ("src_slot", "<u4"), ("via_slot", "<u4"),
                                 ("nresolved", "<u4"), ("role", "u1"), ("tier", "u1"), ("state", "u1"), ("issue", "u1"), ("src_state", "u1"), ("src_issue", "u1"),
                                 ("pad", "u1", 2)])

    def _decisions_dev(self, dec):
        """dec: None, a torch device tensor of gys_listener_decision records, or a numpy DECISION_DT array (copied to the device)"""
        if dec is None or isinstance(dec, self.torch.Tensor):
            return dec
        assert dec.dtype == self.DECISION_DT and len(dec) == self.num_services()
        return self.torch.from_numpy(np.frombuffer(np.ascontiguousarray(dec).tobytes(), dtype=np.uint8).copy()).to(self.device)

    @staticmethod
    def _resol_stats(st):
        d = {k: getattr(st, k) for k, _ in capi.SvcResolStats._fields_}
        d["resolved_at_tier"] = list(st.resolved_at_tier)
        return d

    def resolve_issues_dev(self, dec=None, max_tiers=0, impact=True):
        """gys_svc_resolve_issues_dev -> (torch uint8 device tensor [num_services, 16]: the gys_svc_resol record of every slot; torch float64
        device tensor [num_services]: nresolved of a source, NaN elsewhere (None with impact=False); the gys_svc_resol_stats as a dict).
        dec = the decisions that replace the kept states (see _decisions_dev)"""
        n = max(self.num_services(), 1)
        d_dec = self._decisions_dev(dec)
        out = self.torch.zeros((n, 16), dtype=self.torch.uint8, device=self.device)
        imp = self.torch.zeros(n, dtype=self.torch.float64, device=self.device) if impact else None
        st = capi.SvcResolStats()
        self.order()
        capi.check(self.L.gys_svc_resolve_issues_dev(self.h, C.c_void_p(d_dec.data_ptr()) if d_dec is not None else None, max_tiers, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(imp.data_ptr()) if impact else None, C.byref(st)))
        return out, imp, self._resol_stats(st)

    def resolve_issues_np(self, dec=None, max_tiers=0):
        """resolve_issues_dev copied to the host -> (numpy SVC_RESOL_DT array [num_services], numpy float64 impact column, stats)"""
        out, imp, st = self.resolve_issues_dev(dec, max_tiers)
        self.sync()
        n = self.num_services()
        return np.frombuffer(out.cpu().numpy().tobytes(), dtype=self.SVC_RESOL_DT)[:n].copy(), imp.cpu().numpy()[:n].copy(), st

    def resolve_issues(self, dec=None, max_tiers=0, role_mask=0, cap=None):
        """gys_svc_resolve_issues -> (rc, rows as a numpy SVC_RESOL_ROW_DT array in slot order, number of matches, stats); role_mask bit r
        lists role r (0 = roles 1 .. 4); rc is capi.ERR_NOMEM (and the array empty) when more match than cap.  cap None = num_services"""
        if cap is None:
            cap = self.num_services()
        d_dec = self._decisions_dev(dec)
        out = (capi.SvcResolRow * max(cap, 1))()
        nout, nmatch, st = C.c_uint32(), C.c_uint32(), capi.SvcResolStats()
        self.order()
        rc = self.L.gys_svc_resolve_issues(self.h, C.c_void_p(d_dec.data_ptr()) if d_dec is not None else None, max_tiers, role_mask, out, cap, C.byref(nout),
                                           C.byref(nmatch), C.byref(st))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        return rc, np.frombuffer(out, dtype=self.SVC_RESOL_ROW_DT, count=nout.value).copy(), nmatch.value, self._resol_stats(st)

    def handle_comm_stream(self, machine_id, stream_bytes):
        """L1 + L2 of madhava for one partha connection: COMM_HEADER-framed messages -> partha_tcp_conn_info / partha_listener_state"""
        buf = np.frombuffer(stream_bytes, dtype=np.uint8)
        buf = np.require(buf, requirements=["A", "C"])
        st = capi.CommStats()
        capi.check(self.L.gys_ingest_comm_stream(self.h, mid_buf(machine_id), C.c_void_p(buf.ctypes.data), len(buf), C.byref(st)))
        return st

    def handle_host_state(self, machine_id, ntasks_issue=0, ntasks=0, nlisten_issue=0, nlisten=0, cpu_issue=0, mem_issue=0, curr_state=1):
        st = capi.HostState(ntasks_issue, ntasks, nlisten_issue, nlisten, cpu_issue, mem_issue, curr_state, 0)
        capi.check(self.L.gys_ingest_host_state(self.h, mid_buf(machine_id), C.byref(st)))

    # ---------------------------------------------------------------- window boundary
    def reduce_sections(self):
        if self._sections is None:
            secs = (capi.ReduceSection * 4)()
            n = C.c_uint32()
            capi.check(self.L.gys_reduce_sections(self.h, secs, C.byref(n)))
            out = []
            if self.arena is not None:
                base = self.arena.data_ptr()
                dts = _torch_dtypes()
                for i in range(n.value):
                    s = secs[i]
                    esz = {0: 1, 1: 4, 2: 8}[s.dtype]
                    off = s.dev_ptr - base
                    out.append((self.arena[off:off + s.nelems * esz].view(dts[s.dtype]), s.op))
            self._sections = out
        return self._sections

    def send_cluster_state(self, tusec=0, group=None):
        """MCONN_HANDLER::send_cluster_state + SHCONN_HANDLER::aggregate_cluster_state: close the window on every rank."""
        if self.nranks <= 1:  # the whole boundary as one captured hipGraph (gys_window_close)
            capi.check(self.L.gys_window_close(self.h, tusec))
            return
        capi.check(self.L.gys_window_prepare(self.h, tusec))
        if self.nranks > 1:
            if self.arena is None:
                raise RuntimeError("multi-rank reduce needs torch_arena=True")
            with self.torch.cuda.stream(self.stream):  # the collectives read / write the arena in the engine stream's order
                allreduce_sections(self.reduce_sections(), group)
        capi.check(self.L.gys_window_finish(self.h))

    window_close = send_cluster_state

    # the same boundary with the collectives INSIDE the library (RCCL, no torch in the data path): gys_window_close_rccl
    def join_rccl(self, uid_bytes):
        """uid_bytes: the 128 bytes of gys_rccl_unique_id from rank 0 (every rank must call this; ncclCommInitRank is collective)"""
        uid = (C.c_uint8 * capi.RCCL_UID_BYTES)(*uid_bytes)
        comm = C.c_void_p()
        capi.check(self.L.gys_rccl_comm_create(self.h, uid, max(self.nranks, 1), self.rank, C.byref(comm)))
        self.comm = comm

    def rccl_unique_id(self):
        uid = (C.c_uint8 * capi.RCCL_UID_BYTES)()
        capi.check(self.L.gys_rccl_unique_id(uid))
        return bytes(uid)

    def window_close_rccl(self, tusec=0):
        capi.check(self.L.gys_window_close_rccl(self.h, self.comm, tusec))

    def leave_rccl(self):
        if getattr(self, "comm", None):
            self.sync()
            capi.check(self.L.gys_rccl_comm_destroy(self.comm))
            self.comm = None

    def sync(self):
        capi.check(self.L.gys_sync(self.h))

    # ---------------------------------------------------------------- queries / exports
    def svcsumm(self, machine_id):
        out = capi.SvcSumm()
        capi.check(self.L.gys_query_svcsumm(self.h, mid_buf(machine_id), C.byref(out)))
        return out

    def clusterstate(self, name):
        out = capi.ClusterState()
        capi.check(self.L.gys_query_clusterstate(self.h, name.encode(), C.byref(out)))
        return out

    def scan_quantiles(self, qs):
        """t-digest quantiles of EVERY service in one device pass: [nsvc][len(qs)] float64 (gys_scan_quantiles_dev)"""
        n = self.num_services()
        out = self.torch.empty((max(n, 1), len(qs)), dtype=self.torch.float64, device=self.device)
        qa = (C.c_double * len(qs))(*qs)
        self.order()
        capi.check(self.L.gys_scan_quantiles_dev(self.h, qa, len(qs), C.c_void_p(out.data_ptr())))
        return out[:n].cpu().numpy()

    # ---------------------------------------------------------------- ranks: how many responses finished within x ms ("Ranks" in gysketch.h)
    @staticmethod
    def _thresholds(thr):
        thr = [int(x) for x in thr]
        return (C.c_int64 * max(len(thr), 1))(*thr), len(thr)

    def ranks(self, glob_id, thr):
        """one service (gys_query_ranks): (below [len(thr)] float64, total) -- the same bits as scan_ranks(thr)[0][slot]"""
        ta, nt = self._thresholds(thr)
        below, total = np.zeros(max(nt, 1), dtype=np.float64), C.c_uint64()
        capi.check(self.L.gys_query_ranks(self.h, int(glob_id), ta, nt, below.ctypes.data_as(C.POINTER(C.c_double)), C.byref(total)))
        return below[:nt], total.value

    def scan_ranks(self, thr):
        """EVERY service slot in one device pass (gys_scan_ranks_dev): (below [nsvc][len(thr)] float64, total [nsvc] uint64)"""
        ta, nt = self._thresholds(thr)
        n = self.num_services()
        below = self.torch.empty((max(n, 1), max(nt, 1)), dtype=self.torch.float64, device=self.device)
        total = self.torch.empty(max(n, 1), dtype=self.torch.int64, device=self.device)
        self.order()
        capi.check(self.L.gys_scan_ranks_dev(self.h, ta, nt, C.c_void_p(below.data_ptr()), C.c_void_p(total.data_ptr())))
        self.sync()
        return below[:n].cpu().numpy(), total[:n].cpu().numpy().view(np.uint64)

    def slab_ranks(self, dev_slabs, n, thr):
        """the same for n slabs on the device (gys_tdigest_slab_ranks_dev): roll-ups of any scope, rows of rollup_filtered, a cross-rank
        merge -- (below [n][len(thr)] float64, total [n] uint64)"""
        ta, nt = self._thresholds(thr)
        below = self.torch.empty((max(n, 1), max(nt, 1)), dtype=self.torch.float64, device=self.device)
        total = self.torch.empty(max(n, 1), dtype=self.torch.int64, device=self.device)
        self.order()
        capi.check(self.L.gys_tdigest_slab_ranks_dev(self.h, C.c_void_p(dev_slabs.data_ptr()), n, ta, nt, C.c_void_p(below.data_ptr()), C.c_void_p(total.data_ptr())))
        self.sync()
        return below[:n].cpu().numpy(), total[:n].cpu().numpy().view(np.uint64)

    LSCAN_DT = np.dtype([("glob_id", "<u8"), ("tcount", "<i8", 4), ("tsum", "<i8", 4), ("p95_ms", "<i4", 4), ("p99_ms", "<i4", 4), ("p25_ms", "<i4", 4),
                         ("last_qps", "<i4"), ("curr_qps", "<i4"), ("qps_p95", "<i4"), ("qps_p25", "<i4"), ("act_p95", "<i4"), ("act_p25", "<i4"),
                         ("b5", "u1"), ("b300", "u1"), ("b5day", "u1"), ("nconn_active", "u1"), ("nactive_conn_arr", "u1", 15), ("reserved", "u1", 5)])
    assert LSCAN_DT.itemsize == 168

    def scan_listener_state(self, tusec, qps_multiple=1.0, diffsec=5):
        """the per-listener 5-s scan from the engine's own state (gys_scan_listener_state_dev): (device tensor of the 88-byte
        LISTENER_STATE_NOTIFY records, the same as a numpy record array, the gys_listener_scan records)"""
        n = self.num_services()
        notify = self.torch.zeros(max(n, 1) * 88, dtype=self.torch.uint8, device=self.device)
        scan = self.torch.zeros(max(n, 1) * self.LSCAN_DT.itemsize, dtype=self.torch.uint8, device=self.device)
        self.order()
        capi.check(self.L.gys_scan_listener_state_dev(self.h, int(tusec), float(qps_multiple), int(diffsec), C.c_void_p(notify.data_ptr()),
                                                      C.c_void_p(scan.data_ptr())))
        self.sync()
        return (notify, np.frombuffer(notify.cpu().numpy().tobytes(), dtype=wire.LISTENER_STATE_NOTIFY)[:n],
                np.frombuffer(scan.cpu().numpy().tobytes(), dtype=self.LSCAN_DT)[:n])

    ISSUE_IN_DT = np.dtype([("ser_errors", "<u4"), ("tasks_delay_msec", "<u4"), ("tasks_cpudelay_msec", "<u4"), ("tasks_blkiodelay_msec", "<u4"), ("nconn", "<i4"),
                            ("ntasks_issue", "<u2"), ("ntasks_noissue", "<u2"), ("flags", "u1"), ("pad", "u1", 7), ("tdiff_start", "<i8")])  # (the C struct's int64 sits at offset 32)
    DECISION_DT = np.dtype([("state", "u1"), ("issue", "u1"), ("issue_bit_hist", "u1"), ("high_resp_bit_hist", "u1"), ("decided_line", "<u2"), ("pad", "<u2")])

    def decide_listener_state(self, scan_np, issue_in=None, notify_dev=None):
        """TCP_LISTENER::get_curr_state for every listener (gys_decide_listener_state_dev): scan_np = the gys_listener_scan records (numpy, LSCAN_DT),
        issue_in = numpy ISSUE_IN_DT array or None, notify_dev = the scan's device tensor of 88-byte records (patched in place) or None.
        Returns the gys_listener_decision records (numpy)."""
        n = len(scan_np)
        assert self.ISSUE_IN_DT.itemsize == 40 and self.DECISION_DT.itemsize == 8
        d_scan = self.torch.from_numpy(np.frombuffer(np.ascontiguousarray(scan_np).tobytes(), dtype=np.uint8).copy()).to(self.device)
        d_in = None
        if issue_in is not None:
            assert issue_in.dtype == self.ISSUE_IN_DT and len(issue_in) == n
            d_in = self.torch.from_numpy(np.frombuffer(np.ascontiguousarray(issue_in).tobytes(), dtype=np.uint8).copy()).to(self.device)
        d_out = self.torch.zeros(max(n, 1) * 8, dtype=self.torch.uint8, device=self.device)
        self.order()
        capi.check(self.L.gys_decide_listener_state_dev(self.h, C.c_void_p(d_scan.data_ptr()), C.c_void_p(d_in.data_ptr() if d_in is not None else None),
                                                        C.c_void_p(notify_dev.data_ptr() if notify_dev is not None else None), C.c_void_p(d_out.data_ptr())))
        self.sync()
        return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=self.DECISION_DT)[:n]

    SLAB_DT = np.dtype([("sum", "<i8", capi.TD_NB), ("cnt", "<u8", capi.TD_NB), ("vmin", "<i8"), ("vmax", "<i8")])

    def tdigest_rollup(self, scope):
        """roll-up digests (gys_tdigest_rollup_dev): torch uint8 tensor of n slabs on the device + the same as a numpy record array"""
        n = {capi.ROLLUP_HOST: self.L.gys_num_hosts(self.h), capi.ROLLUP_CLUSTER: self.L.gys_num_clusters(self.h), capi.ROLLUP_GLOBAL: 1}[scope]
        dev = self.torch.zeros(max(n, 1) * C.sizeof(capi.TDigestSlab), dtype=self.torch.uint8, device=self.device)
        self.order()
        capi.check(self.L.gys_tdigest_rollup_dev(self.h, scope, C.c_void_p(dev.data_ptr())))
        self.sync()
        return dev, np.frombuffer(dev.cpu().numpy().tobytes(), dtype=self.SLAB_DT)[:n]

    def tdigest_merge_slabs(self, dev_slabs, n):
        out = self.torch.zeros(C.sizeof(capi.TDigestSlab), dtype=self.torch.uint8, device=self.device)
        self.order()
        capi.check(self.L.gys_tdigest_merge_slabs_dev(self.h, C.c_void_p(dev_slabs.data_ptr()), n, C.c_void_p(out.data_ptr())))
        self.sync()
        return out, np.frombuffer(out.cpu().numpy().tobytes(), dtype=self.SLAB_DT)[0]

    # ---------------------------------------------------------------- distinct-flow counts from the per-service HyperLogLog registers (svc_hll_p)
    def scan_distinct(self):
        """the distinct-flow estimate of EVERY service in one device pass: [nsvc] float64 (gys_scan_distinct_dev; the open window)"""
        n = self.num_services()
        out = self.torch.zeros(max(n, 1), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_scan_distinct_dev(self.h, C.c_void_p(out.data_ptr())))
        self.sync()
        return out[:n].cpu().numpy()

    def query_distinct(self, glob_id):
        """one service's distinct-flow estimate (gys_query_distinct): the same bits as scan_distinct()[slot]"""
        out = C.c_double()
        capi.check(self.L.gys_query_distinct(self.h, int(glob_id), C.byref(out)))
        return out.value

    def _hll_groups(self, scope):
        return {capi.ROLLUP_HOST: self.L.gys_num_hosts(self.h), capi.ROLLUP_CLUSTER: self.L.gys_num_clusters(self.h), capi.ROLLUP_GLOBAL: 1}.get(scope, 1)

    def hll_rollup(self, scope, want_regs=True):
        """register files and estimates of the hosts / clusters / the rank (gys_hll_rollup_dev): (files (ngroups, m) uint8 or None when
        want_regs is False, estimates (ngroups,) float64)"""
        n, m = self._hll_groups(scope), self.L.gys_hll_file_bytes(self.h)
        regs = self.torch.zeros(max(n * m, 16), dtype=self.torch.uint8, device=self.device) if want_regs else None
        est = self.torch.zeros(max(n, 1), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_hll_rollup_dev(self.h, scope, C.c_void_p(regs.data_ptr()) if want_regs else None, C.c_void_p(est.data_ptr())))
        self.sync()
        return (regs[:n * m].cpu().numpy().reshape(n, m) if want_regs else None), est[:n].cpu().numpy()

    def hll_merge_files(self, regs):
        """the union of register files (numpy (n, m) uint8, or a torch uint8 device tensor of n * m bytes) and its estimate
        (gys_hll_merge_files_dev): ((m,) uint8, float)"""
        m = self.L.gys_hll_file_bytes(self.h)
        if not self.torch.is_tensor(regs):
            regs = self.torch.from_numpy(np.ascontiguousarray(regs, dtype=np.uint8).reshape(-1)).to(self.device)
        n = regs.numel() // m if m else 0
        out = self.torch.zeros(max(m, 16), dtype=self.torch.uint8, device=self.device)
        est = self.torch.zeros(1, dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_hll_merge_files_dev(self.h, C.c_void_p(regs.data_ptr()), n, C.c_void_p(out.data_ptr()), C.c_void_p(est.data_ptr())))
        self.sync()
        return out[:m].cpu().numpy(), float(est.cpu().numpy()[0])

    def hll_global_rccl(self):
        """the all-rank register file and its estimate (gys_hll_global_rccl; join_rccl first): ((m,) uint8, float), the same on every rank"""
        m = self.L.gys_hll_file_bytes(self.h)
        out = self.torch.zeros(max(m, 16), dtype=self.torch.uint8, device=self.device)
        est = self.torch.zeros(1, dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_hll_global_rccl(self.h, self.comm, C.c_void_p(out.data_ptr()), C.c_void_p(est.data_ptr())))
        self.sync()
        return out[:m].cpu().numpy(), float(est.cpu().numpy()[0])

    # ---------------------------------------------------------------- ... of the CLOSED windows, per level (svc_hll_levels; 0 = window closed last, 1 = 300 s, 2 = 5 days, 3 = all)
    def scan_distinct_level(self, level, tusec=0):
        """the level's distinct-flow estimate of EVERY service at time tusec: [nsvc] float64 (gys_scan_distinct_level_dev)"""
        n = self.num_services()
        out = self.torch.zeros(max(n, 1), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_scan_distinct_level_dev(self.h, level, tusec, C.c_void_p(out.data_ptr())))
        self.sync()
        return out[:n].cpu().numpy()

    def query_distinct_level(self, glob_id, level, tusec=0):
        """one service (gys_query_distinct_level): the same bits as scan_distinct_level(level, tusec)[slot]"""
        out = C.c_double()
        capi.check(self.L.gys_query_distinct_level(self.h, int(glob_id), level, tusec, C.byref(out)))
        return out.value

    def hll_rollup_level(self, scope, level, tusec=0, want_regs=True):
        """hll_rollup() of a level's files (gys_hll_rollup_level_dev): (files (ngroups, m) uint8 or None, estimates (ngroups,) float64)"""
        n, m = self._hll_groups(scope), self.L.gys_hll_file_bytes(self.h)
        regs = self.torch.zeros(max(n * m, 16), dtype=self.torch.uint8, device=self.device) if want_regs else None
        est = self.torch.zeros(max(n, 1), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_hll_rollup_level_dev(self.h, scope, level, tusec, C.c_void_p(regs.data_ptr()) if want_regs else None, C.c_void_p(est.data_ptr())))
        self.sync()
        return (regs[:n * m].cpu().numpy().reshape(n, m) if want_regs else None), est[:n].cpu().numpy()

    def export_svc_hll_level(self, level, tusec=0, first=0, n=None):
        """the level's register files of slots [first, first + n) at time tusec: (n, m) uint8 (gys_export_svc_hll_level)"""
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 1 << self.cfg.svc_hll_p), dtype=np.uint8)
        capi.check(self.L.gys_export_svc_hll_level(self.h, level, tusec, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def slab_quantiles(self, dev_slab, qs, index=0):
        qa = (C.c_double * len(qs))(*qs)
        out = (C.c_double * len(qs))()
        capi.check(self.L.gys_tdigest_slab_quantiles(self.h, C.c_void_p(dev_slab.data_ptr() + index * C.sizeof(capi.TDigestSlab)), qa, len(qs), out))
        return list(out)

    def slab_quantiles_dev(self, dev_slabs, n, qs):
        """quantiles of n slabs on the device in one launch (gys_tdigest_slab_quantiles_dev): (device tensor [n][len(qs)] float64, the same as
        numpy) -- every entry the bits slab_quantiles gives for that slab and quantile"""
        qa = (C.c_double * max(len(qs), 1))(*qs)
        out = self.torch.empty((max(n, 1), max(len(qs), 1)), dtype=self.torch.float64, device=self.device)
        self.order()
        capi.check(self.L.gys_tdigest_slab_quantiles_dev(self.h, C.c_void_p(dev_slabs.data_ptr()), n, qa, len(qs), C.c_void_p(out.data_ptr())))
        self.sync()
        return out, out[:n].cpu().numpy()

    TOPK_DT = np.dtype([("row", "<u4"), ("reserved", "<u4"), ("value", "<f8"), ("weight", "<u8")])
    TOPSVC_DT = np.dtype([("glob_id", "<u8"), ("slot", "<u4"), ("host_slot", "<u4"), ("value", "<f8"), ("total", "<u8")])

    def topk(self, col, k, order=capi.TOPK_LARGEST, stride=1, rows=None, weight=None, min_weight=0, nrows=None):
        """exact top-k of a device column of doubles (gys_topk_dev; "Top-k" in gysketch.h): col = torch float64 device tensor, rows = torch
        int32 device tensor of distinct row numbers or None (rows 0 .. nrows - 1; nrows defaults to col.numel() // stride), weight = torch
        int64 device tensor indexed by row or None.  -> (entries as a numpy TOPK_DT array, in order; number of eligible rows)"""
        if nrows is None:
            nrows = rows.numel() if rows is not None else col.numel() // max(stride, 1)
        out = (capi.TopkEntry * max(k, 1))()
        nout, nel = C.c_uint32(), C.c_uint64()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.order()
        capi.check(self.L.gys_topk_dev(self.h, ptr(col), stride, nrows, ptr(rows), ptr(weight), int(min_weight), order, k, out, C.byref(nout), C.byref(nel)))
        return np.frombuffer(out, dtype=self.TOPK_DT, count=nout.value).copy(), nel.value

    def top_services(self, metric, param=0.0, k=10, order=capi.TOPK_LARGEST, level=-1, tusec=0, min_total=0, terms=None, group_oper=(), top_oper="and",
                     machine_ids=None, svcids=None, clusters=None, any_state=False, filtered=None):
        """the service ranking in one call (gys_top_services): metric = capi.TOP_*, the filter arguments of rollup_filtered (no filter argument
        at all, or filtered=False: every registered service).  -> (entries as a numpy TOPSVC_DT array, in order; number of eligible services)"""
        if filtered is None:
            filtered = bool(terms or machine_ids or clusters or any_state) or svcids is not None
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        out = (capi.TopService * max(k, 1))()
        nout, nel = C.c_uint32(), C.c_uint64()
        self.order()
        capi.check(self.L.gys_top_services(self.h, metric, float(param), level, int(tusec), C.byref(f) if filtered else None, capi.RF_ANY_STATE if any_state else 0,
                                           int(min_total), order, k, out, C.byref(nout), C.byref(nel)))
        return np.frombuffer(out, dtype=self.TOPSVC_DT, count=nout.value).copy(), nel.value

    def hist_percentiles(self, glob_id, pcts, which=1):
        pd = (capi.HistData * len(pcts))()
        for i, p in enumerate(pcts):
            pd[i].percentile = p
        total, maxv, avg = C.c_uint64(), C.c_int64(), C.c_float()
        capi.check(self.L.gys_query_hist_percentiles(self.h, int(glob_id), which, pd, len(pcts), C.byref(total), C.byref(maxv), C.byref(avg)))
        return [d.data_value for d in pd], [d.sum for d in pd], [d.count for d in pd], total.value, maxv.value, avg.value

    def quantiles(self, glob_id, qs):
        q = (C.c_double * len(qs))(*qs)
        out = (C.c_double * len(qs))()
        capi.check(self.L.gys_query_quantiles(self.h, int(glob_id), q, len(qs), out))
        return list(out)

    def distinct_flows(self):
        out = C.c_double()
        capi.check(self.L.gys_query_distinct_flows(self.h, C.byref(out)))
        return out.value

    def cms(self, glob_id, which=0):
        out = C.c_uint64()
        capi.check(self.L.gys_query_cms(self.h, int(glob_id), which, C.byref(out)))
        return out.value

    def topn(self, machine_id, kind):
        out = (capi.TopnEntry * capi.TOPN)()
        n = C.c_uint32()
        capi.check(self.L.gys_query_topn(self.h, mid_buf(machine_id), kind, out, C.byref(n)))
        return [(out[i].glob_id, out[i].metric, bytes(out[i].state)) for i in range(n.value)]

    def _json(self, fn, *args):
        """two-call pattern: ask for the size, then fetch"""
        need = C.c_size_t()
        rc = fn(self.h, *args, None, 0, C.byref(need))
        if rc not in (capi.OK, capi.ERR_NOMEM):
            capi.check(rc)
        buf = C.create_string_buffer(need.value + 1)
        capi.check(fn(self.h, *args, buf, need.value + 1, C.byref(need)))
        return buf.value.decode()

    def set_host_name(self, machine_id, hostname):
        capi.check(self.L.gys_set_host_name(self.h, mid_buf(machine_id), hostname.encode()))

    def json_svcsumm(self, machine_id, madid="0" * 16, timestr=""):
        return self._json(self.L.gys_json_svcsumm, mid_buf(machine_id), madid.encode(), timestr.encode())

    def json_svcstate(self, machine_id, madid="0" * 16, timestr=""):
        return self._json(self.L.gys_json_svcstate, mid_buf(machine_id), madid.encode(), timestr.encode())

    def json_toplisteners(self, machine_id=None, flags=15, madid="0" * 16, timestr=""):
        """web_curr_top_listeners; machine_id None = the multi-host form (50 slots per kind over all hosts)"""
        m = mid_buf(machine_id) if machine_id is not None else None
        return self._json(self.L.gys_json_toplisteners, m, flags, madid.encode(), timestr.encode())

    def json_svcsumm_multihost(self, terms=None, group_oper=(), top_oper="and", sort_col=None, sort_desc=True, maxrecs=1 << 30, machine_ids=None,
                               clusters=None, madid="0" * 16, timestr=""):
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, None, clusters, cols=capi.SUMM_COLS)
        return self._json(self.L.gys_json_svcsumm_multihost, C.byref(f), -1 if sort_col is None else capi.SUMM_COLS.index(sort_col), 1 if sort_desc else 0,
                          maxrecs, madid.encode(), timestr.encode())

    def _svc_filter(self, terms, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None, cols=None):
        """terms: [(column name, comparator, value or list of values, group = 0)]; group_oper: per group "and" / "or"; -> (SvcFilter, keep-alive)"""
        terms = list(terms or [])
        arr = (capi.SvcTerm * max(len(terms), 1))()
        setv = []
        for i, t in enumerate(terms):
            col, comp, val = t[0], t[1], t[2]
            arr[i].col = (cols or capi.SVC_COLS).index(col)
            arr[i].comp = capi.COMP[comp]
            arr[i].group = t[3] if len(t) > 3 else 0
            if comp in ("in", "notin"):
                arr[i].set_first = len(setv)
                arr[i].nvalues = len(val)
                setv += [int(v) for v in val]
            elif comp not in ("bit2", "bit3"):
                arr[i].value = int(val)
        f = capi.SvcFilter()
        f.terms = arr
        f.nterms = len(terms)
        sv = (C.c_int64 * max(len(setv), 1))(*setv)
        f.set_values = sv
        f.nset_values = len(setv)
        for g, o in enumerate(group_oper):
            f.group_oper[g] = 1 if o == "or" else 0
        f.top_oper = 1 if top_oper == "or" else 0
        mids = None
        if machine_ids:
            mids = (C.c_uint8 * (16 * len(machine_ids)))(*b"".join(machine_ids))
            f.machine_ids = mids
            f.nmachine_ids = len(machine_ids)
        ids = cl = None
        if svcids is not None and len(svcids):
            ids = (C.c_uint64 * len(svcids))(*[int(x) for x in svcids])
            f.svcids = ids
            f.nsvcids = len(svcids)
        if clusters:
            cl = (C.c_char_p * len(clusters))(*[x.encode() for x in clusters])
            f.clusters = cl
            f.nclusters = len(clusters)
        return f, (arr, sv, mids, ids, cl)

    def svcstate_percentiles(self, col, pcts, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None):
        """gys_query_svcstate_percentiles -> (values (int64 array), number matched)"""
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        p = np.ascontiguousarray(pcts, dtype=np.float64)
        out = np.zeros(len(p), dtype=np.int64)
        nm = C.c_uint64()
        capi.check(self.L.gys_query_svcstate_percentiles(self.h, C.byref(f), capi.SVC_COLS.index(col), p.ctypes.data_as(capi.f64p), len(p),
                                                          out.ctypes.data_as(capi.i64p), C.byref(nm)))
        return out, nm.value

    def svc_ids_by_name(self, comp, patterns):
        """gys_svc_ids_by_name: glob_ids of the registered services whose process name matches the string criterion (for svcids=...)"""
        pats = [patterns] if isinstance(patterns, (str, bytes)) else list(patterns)
        arr = (C.c_char_p * len(pats))(*[p if isinstance(p, bytes) else p.encode() for p in pats])
        cap = max(self.num_services(), 1)
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_uint32()
        capi.check(self.L.gys_svc_ids_by_name(self.h, capi.COMP[comp], arr, len(pats), out.ctypes.data_as(capi.u64p), cap, C.byref(n)))
        return out[:n.value].copy()

    def machine_ids_by_hostname(self, comp, patterns):
        """gys_machine_ids_by_hostname: machine ids (16 bytes each) of the registered hosts whose name matches (for machine_ids=...)"""
        pats = [patterns] if isinstance(patterns, (str, bytes)) else list(patterns)
        arr = (C.c_char_p * len(pats))(*[p if isinstance(p, bytes) else p.encode() for p in pats])
        cap = 1 << 16
        out = np.zeros(cap * 16, dtype=np.uint8)
        n = C.c_uint32()
        capi.check(self.L.gys_machine_ids_by_hostname(self.h, capi.COMP[comp], arr, len(pats), out.ctypes.data_as(capi.u8p), cap, C.byref(n)))
        return [out[16 * i:16 * i + 16].tobytes() for i in range(n.value)]

    def svcstate_scan(self, terms=None, group_oper=(), top_oper="and", sort_col=None, sort_desc=True, maxrecs=1000, machine_ids=None, svcids=None,
                      clusters=None):
        """gys_query_svcstate_scan -> (slots, host slots, records as a numpy array of wire.LISTENER_STATE_NOTIFY, number matched)"""
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        out = (capi.SvcRow * max(maxrecs, 1))()
        nout, nm = C.c_uint32(), C.c_uint64()
        capi.check(self.L.gys_query_svcstate_scan(self.h, C.byref(f), -1 if sort_col is None else capi.SVC_COLS.index(sort_col), 1 if sort_desc else 0,
                                                  maxrecs, out, C.byref(nout), C.byref(nm)))
        raw = np.frombuffer(out, dtype=np.uint8, count=nout.value * 96).reshape(nout.value, 96)
        slots = raw[:, 0:4].copy().view(np.uint32).ravel()
        hosts = raw[:, 4:8].copy().view(np.uint32).ravel()
        recs = raw[:, 8:96].copy().view(wire.LISTENER_STATE_NOTIFY).ravel()
        return slots, hosts, recs, nm.value

    def json_svcstate_multihost(self, terms=None, group_oper=(), top_oper="and", sort_col=None, sort_desc=True, maxrecs=1000, machine_ids=None,
                                madid="0" * 16, timestr=""):
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids)
        return self._json(self.L.gys_json_svcstate_multihost, C.byref(f), -1 if sort_col is None else capi.SVC_COLS.index(sort_col), 1 if sort_desc else 0,
                          maxrecs, madid.encode(), timestr.encode())

    def svcstate_aggr(self, cols, group_by=0, terms=None, group_oper=(), top_oper="and", machine_ids=None, maxrows=None, svcids=None, clusters=None):
        """gys_query_svcstate_aggr -> list of (group, count, {col: (sum, min, max)})"""
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        ca = (C.c_uint8 * max(len(cols), 1))(*[capi.SVC_COLS.index(c) for c in cols])
        if maxrows is None:
            maxrows = 1 if group_by == 0 else 1 << 16
        out = (capi.SvcAggrRow * max(maxrows, 1))()
        n = C.c_uint32()
        capi.check(self.L.gys_query_svcstate_aggr(self.h, C.byref(f), group_by, ca, len(cols), out, maxrows, C.byref(n)))
        res = []
        for i in range(min(n.value, maxrows)):
            r = out[i]
            res.append((r.group, r.count, {c: (r.sum[a], r.min[a], r.max[a]) for a, c in enumerate(cols)}))
        return res

    # ---------------------------------------------------------------- roll-up digests / distinct counts of the services a filter selects, per group
    def set_service_groups(self, glob_ids, groups):
        """gys_set_service_groups: the caller's dense group index (or capi.NO_GROUP) per service; all-or-nothing on an unknown id"""
        ids = np.ascontiguousarray(glob_ids, dtype=np.uint64)
        grp = np.ascontiguousarray(groups, dtype=np.uint32)
        assert ids.shape == grp.shape and ids.ndim == 1
        capi.check(self.L.gys_set_service_groups(self.h, ids.ctypes.data_as(capi.u64p), grp.ctypes.data_as(capi.u32p), len(ids)))
        real = grp[grp != capi.NO_GROUP]
        if len(real):  # the label domain: what rollup_filtered sizes its outputs by (the library keeps 64 KB of scratch per computed row)
            self._label_domain = max(getattr(self, "_label_domain", 0), int(real.max()) + 1)

    def rollup_filtered(self, group_by=0, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None, any_state=False,
                        hll_level=-1, tusec=0, want=("slabs", "regs", "est"), maxrows=None):
        """gys_rollup_filtered_dev -> (rows [(group, nmembers)] of the groups written, nrows there are, {"slabs": SLAB_DT records,
        "regs": (rows, m) uint8, "est": (rows,) float64} for the outputs named in `want`)"""
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        if maxrows is None:
            maxrows = {capi.GROUP_NONE: 1, capi.GROUP_HOST: self.L.gys_num_hosts(self.h), capi.GROUP_CLUSTER: self.L.gys_num_clusters(self.h)}.get(
                group_by, min(getattr(self, "_label_domain", 0), self.num_services()))
        cap = max(maxrows, 1)
        m = self.L.gys_hll_file_bytes(self.h)
        u8 = self.torch.uint8
        slabs = self.torch.zeros(cap * C.sizeof(capi.TDigestSlab), dtype=u8, device=self.device) if "slabs" in want else None
        regs = self.torch.zeros(max(cap * m, 16), dtype=u8, device=self.device) if "regs" in want else None
        est = self.torch.zeros(cap, dtype=self.torch.float64, device=self.device) if "est" in want else None
        rows = (capi.RollupRow * cap)()
        n = C.c_uint32()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.order()
        capi.check(self.L.gys_rollup_filtered_dev(self.h, C.byref(f), capi.RF_ANY_STATE if any_state else 0, group_by, hll_level, tusec, rows, maxrows,
                                                  C.byref(n), ptr(slabs), ptr(regs), ptr(est)))
        self.sync()
        nr = min(n.value, maxrows)
        out = {}
        if slabs is not None:
            out["slabs"] = np.frombuffer(slabs.cpu().numpy().tobytes(), dtype=self.SLAB_DT)[:nr]
            out["slabs_dev"] = slabs
        if regs is not None:
            out["regs"] = regs[:nr * m].cpu().numpy().reshape(nr, m)
        if est is not None:
            out["est"] = est[:nr].cpu().numpy()
        return [(rows[i].group, rows[i].nmembers) for i in range(nr)], n.value, out

    # ---------------------------------------------------------------- group response-time histograms of the levels (0 = window closed last, 1 = 300 s, 2 = 5 days, 3 = all)
    def _group_percentiles(self, dev_recs, n, pcts):
        """gys_hist_percentiles_dev(GYS_RESP_TIME_HASH) on n device records: (n, len(pcts)) int64"""
        out = self.torch.zeros(max(n * len(pcts), 1), dtype=self.torch.int64, device=self.device)
        pa = (C.c_float * len(pcts))(*pcts)
        capi.check(self.L.gys_hist_percentiles_dev(self.h, 0, C.c_void_p(dev_recs.data_ptr()), n, pa, len(pcts), C.c_void_p(out.data_ptr())))
        self.sync()
        return out[:n * len(pcts)].cpu().numpy().reshape(n, len(pcts))

    def hist_rollup_level(self, scope, level, tusec=0, pcts=None):
        """gys_hist_rollup_level_dev: the hosts' / clusters' / the rank's records of a level at tusec, [groups][16][2] int64 like
        export_hist_level; with pcts=(...) -> (records, percentiles (groups, len(pcts)) int64 of gys_hist_percentiles_dev on the device records)"""
        n = self._hll_groups(scope)
        recs = self.torch.zeros((max(n, 1), 16, 2), dtype=self.torch.int64, device=self.device)
        self.order()
        capi.check(self.L.gys_hist_rollup_level_dev(self.h, scope, level, int(tusec), C.c_void_p(recs.data_ptr())))
        self.sync()
        out = recs[:n].cpu().numpy()
        return out if pcts is None else (out, self._group_percentiles(recs, n, pcts))

    def hist_rollup_filtered(self, group_by=0, level=3, tusec=0, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None,
                             any_state=False, maxrows=None, pcts=None):
        """gys_hist_rollup_filtered_dev -> (rows [(group, nmembers)] of the groups written, nrows there are, records [rows][16][2] int64); with
        pcts=(...) a fourth element: the rows' percentiles (rows, len(pcts)) int64"""
        f, keep = self._svc_filter(terms, group_oper, top_oper, machine_ids, svcids, clusters)
        if maxrows is None:
            maxrows = {capi.GROUP_NONE: 1, capi.GROUP_HOST: self.L.gys_num_hosts(self.h), capi.GROUP_CLUSTER: self.L.gys_num_clusters(self.h)}.get(
                group_by, min(getattr(self, "_label_domain", 0), self.num_services()))
        cap = max(maxrows, 1)
        recs = self.torch.zeros((cap, 16, 2), dtype=self.torch.int64, device=self.device)
        rows = (capi.RollupRow * cap)()
        n = C.c_uint32()
        self.order()
        capi.check(self.L.gys_hist_rollup_filtered_dev(self.h, C.byref(f), capi.RF_ANY_STATE if any_state else 0, group_by, level, int(tusec), rows, maxrows,
                                                       C.byref(n), C.c_void_p(recs.data_ptr())))
        self.sync()
        nr = min(n.value, maxrows)
        res = ([(rows[i].group, rows[i].nmembers) for i in range(nr)], n.value, recs[:nr].cpu().numpy())
        return res if pcts is None else res + (self._group_percentiles(recs, nr, pcts),)

    # ---------------------------------------------------------------- group records of any period, group QPS / active-connection histograms, day statistics per group
    def _filtered_call(self, fn, group_by, filt, any_state, maxrows, out_of, *mid):
        """the rows / maxrows / nrows part the filtered group calls share: fn(h, filter, flags, group_by, *mid, rows, maxrows, &nrows, out, ...);
        out_of(cap) -> (device tensor, trailing arguments).  Returns (rows, nrows there are, rows written, tensor)"""
        f, keep = self._svc_filter(*filt)
        if maxrows is None:
            maxrows = {capi.GROUP_NONE: 1, capi.GROUP_HOST: self.L.gys_num_hosts(self.h), capi.GROUP_CLUSTER: self.L.gys_num_clusters(self.h)}.get(
                group_by, min(getattr(self, "_label_domain", 0), self.num_services()))
        cap = max(maxrows, 1)
        out, trail = out_of(cap)
        rows = (capi.RollupRow * cap)()
        n = C.c_uint32()
        self.order()
        capi.check(fn(self.h, C.byref(f), capi.RF_ANY_STATE if any_state else 0, group_by, *mid, rows, maxrows, C.byref(n), C.c_void_p(out.data_ptr()), *trail))
        self.sync()
        nr = min(n.value, maxrows)
        return [(rows[i].group, rows[i].nmembers) for i in range(nr)], n.value, nr, out

    def _recs(self, cap):
        return self.torch.zeros((cap, 16, 2), dtype=self.torch.int64, device=self.device)

    def _pcts_of(self, dev_recs, n, pcts, kind):
        out = self.torch.zeros(max(n * len(pcts), 1), dtype=self.torch.int64, device=self.device)
        pa = (C.c_float * len(pcts))(*pcts)
        capi.check(self.L.gys_hist_percentiles_dev(self.h, kind, C.c_void_p(dev_recs.data_ptr()), n, pa, len(pcts), C.c_void_p(out.data_ptr())))
        self.sync()
        return out[:n * len(pcts)].cpu().numpy().reshape(n, len(pcts))

    def hist_rollup_period(self, scope, starttime, endtime, tusec, pcts=None):
        """gys_hist_rollup_period_dev: the hosts' / clusters' / the rank's records of the seconds [starttime, endtime] as of tusec ->
        (records [groups][16][2] int64 like export_hist_period, level that answered); with pcts=(...) a third element: their percentiles
        (groups, len(pcts)) int64 of gys_hist_percentiles_dev on the device records"""
        n = self._hll_groups(scope)
        recs = self._recs(max(n, 1))
        lv = C.c_int(-1)
        self.order()
        capi.check(self.L.gys_hist_rollup_period_dev(self.h, scope, int(starttime), int(endtime), int(tusec), C.c_void_p(recs.data_ptr()), C.byref(lv)))
        self.sync()
        res = (recs[:n].cpu().numpy(), lv.value)
        return res if pcts is None else res + (self._pcts_of(recs, n, pcts, 0),)

    def hist_rollup_period_filtered(self, group_by, starttime, endtime, tusec, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None,
                                    clusters=None, any_state=False, maxrows=None, pcts=None):
        """gys_hist_rollup_period_filtered_dev -> (rows [(group, nmembers)], nrows there are, records [rows][16][2] int64, level that answered);
        with pcts=(...) a fifth element: the rows' percentiles"""
        lv = C.c_int(-1)
        rows, n, nr, recs = self._filtered_call(self.L.gys_hist_rollup_period_filtered_dev, group_by, (terms, group_oper, top_oper, machine_ids, svcids, clusters),
                                                any_state, maxrows, lambda cap: (self._recs(cap), (C.byref(lv),)), int(starttime), int(endtime), int(tusec))
        res = (rows, n, recs[:nr].cpu().numpy(), lv.value)
        return res if pcts is None else res + (self._pcts_of(recs, nr, pcts, 0),)

    @staticmethod
    def _svc_hist_kind(which):
        return capi.KINDS["HASH_1_3000" if which else "SEMI_LOG_HASH_LO"]

    def svc_hist_rollup(self, scope, which, pcts=None):
        """gys_svc_hist_rollup_dev: the groups' QPS (which = 0) / active-connection (1) histograms, [groups][16][2] int64 like export_svc_hist;
        with pcts=(...) -> (records, percentiles by the matching hash kind)"""
        n = self._hll_groups(scope)
        recs = self._recs(max(n, 1))
        self.order()
        capi.check(self.L.gys_svc_hist_rollup_dev(self.h, scope, which, C.c_void_p(recs.data_ptr())))
        self.sync()
        out = recs[:n].cpu().numpy()
        return out if pcts is None else (out, self._pcts_of(recs, n, pcts, self._svc_hist_kind(which)))

    def svc_hist_rollup_filtered(self, group_by, which, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None, any_state=False,
                                 maxrows=None, pcts=None):
        """gys_svc_hist_rollup_filtered_dev -> (rows, nrows there are, records [rows][16][2] int64); with pcts=(...) a fourth element"""
        rows, n, nr, recs = self._filtered_call(self.L.gys_svc_hist_rollup_filtered_dev, group_by, (terms, group_oper, top_oper, machine_ids, svcids, clusters),
                                                any_state, maxrows, lambda cap: (self._recs(cap), ()), which)
        res = (rows, n, recs[:nr].cpu().numpy())
        return res if pcts is None else res + (self._pcts_of(recs, nr, pcts, self._svc_hist_kind(which)),)

    DAY_STATS_DT = np.dtype([("glob_id", "<u8"), ("tcount_5d", "<i8"), ("tsum_5d", "<i8"), ("p95_5d_respms", "<u4"), ("p25_5d_respms", "<u4"), ("p95_qps", "<u4"),
                             ("p25_qps", "<u4"), ("p95_nactive", "<u4"), ("p25_nactive", "<u4")])  # == capi.ListenerDayStats

    def _day_stats(self, cap):
        return self.torch.zeros(cap * self.DAY_STATS_DT.itemsize, dtype=self.torch.uint8, device=self.device)

    def day_stats_rollup(self, scope, tusec):
        """gys_day_stats_rollup_dev: one LISTENER_DAY_STATS per host slot / cluster / the rank as a numpy record array (DAY_STATS_DT)"""
        n = self._hll_groups(scope)
        out = self._day_stats(max(n, 1))
        self.order()
        capi.check(self.L.gys_day_stats_rollup_dev(self.h, scope, int(tusec), C.c_void_p(out.data_ptr())))
        self.sync()
        return np.frombuffer(out.cpu().numpy().tobytes(), dtype=self.DAY_STATS_DT)[:n]

    def day_stats_rollup_filtered(self, group_by, tusec, terms=None, group_oper=(), top_oper="and", machine_ids=None, svcids=None, clusters=None, any_state=False,
                                  maxrows=None):
        """gys_day_stats_rollup_filtered_dev -> (rows, nrows there are, DAY_STATS_DT records of the rows)"""
        rows, n, nr, out = self._filtered_call(self.L.gys_day_stats_rollup_filtered_dev, group_by, (terms, group_oper, top_oper, machine_ids, svcids, clusters),
                                               any_state, maxrows, lambda cap: (self._day_stats(cap), ()), int(tusec))
        return rows, n, np.frombuffer(out.cpu().numpy().tobytes(), dtype=self.DAY_STATS_DT)[:nr]

    def json_clusterstate(self, shyamaid="0" * 16, timestr=""):
        return self._json(self.L.gys_json_clusterstate, shyamaid.encode(), timestr.encode())

    def num_services(self):
        return self.L.gys_num_services(self.h)

    def lookup(self, glob_id):
        s = C.c_uint32()
        capi.check(self.L.gys_lookup_service(self.h, int(glob_id), C.byref(s)))
        return s.value

    def export_hist(self, which, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 16, 2), dtype=np.int64)  # [slot][bucket]{count,sum}; [slot][15] = {total_count, max_val_seen}
        capi.check(self.L.gys_export_hist(self.h, which, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def tdigest_sql_text(self, glob_id):
        """the service's digest as a literal of the Postgres tdigest type ('...'::public.tdigest)"""
        need = C.c_size_t()
        rc = self.L.gys_tdigest_sql_text(self.h, int(glob_id), None, 0, C.byref(need))
        if rc != capi.ERR_NOMEM:
            capi.check(rc)
        buf = C.create_string_buffer(need.value + 1)
        capi.check(self.L.gys_tdigest_sql_text(self.h, int(glob_id), buf, len(buf), C.byref(need)))
        return buf.value.decode()

    def tdigest_sql_binary(self, glob_id):
        need = C.c_size_t()
        rc = self.L.gys_tdigest_sql_binary(self.h, int(glob_id), None, 0, C.byref(need))
        if rc != capi.ERR_NOMEM:
            capi.check(rc)
        buf = C.create_string_buffer(need.value)
        capi.check(self.L.gys_tdigest_sql_binary(self.h, int(glob_id), buf, len(buf), C.byref(need)))
        return buf.raw

    def export_hist_level(self, level, tusec, first=0, n=None):
        """records of one time level (0: last window, 1: 300 s, 2: 5 days, 3: all) as of tusec; same layout as export_hist"""
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 16, 2), dtype=np.int64)
        capi.check(self.L.gys_export_hist_level(self.h, level, int(tusec), first, n, C.c_void_p(out.ctypes.data)))
        return out

    def query_hist_level_stats(self, glob_id, level, tusec, pcts):
        st = (capi.TimeHistVal * len(pcts))()
        for i, p in enumerate(pcts):
            st[i].percentile = p
        tc, ts, mean = C.c_int64(), C.c_int64(), C.c_double()
        capi.check(self.L.gys_query_hist_level_stats(self.h, int(glob_id), level, int(tusec), st, len(pcts), C.byref(tc), C.byref(ts), C.byref(mean)))
        return [s.data_value for s in st], tc.value, ts.value, mean.value

    def export_hist_period(self, starttime, endtime, tusec, first=0, n=None):
        """{count, sum} per histogram bucket of the seconds [starttime, endtime] as TIME_HISTOGRAM::get_stats_for_period sees them
        (common/gy_statistics.h:1378-1406); returns (records [n][16][2], level that answered)"""
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 16, 2), dtype=np.int64)
        lv = C.c_int(-1)
        capi.check(self.L.gys_export_hist_period(self.h, int(starttime), int(endtime), int(tusec), first, n, C.c_void_p(out.ctypes.data), C.byref(lv)))
        return out, lv.value

    def query_hist_period_stats(self, glob_id, starttime, endtime, tusec, pcts):
        st = (capi.TimeHistVal * len(pcts))()
        for i, p in enumerate(pcts):
            st[i].percentile = p
        tc, ts, mean = C.c_int64(), C.c_int64(), C.c_double()
        capi.check(self.L.gys_query_hist_period_stats(self.h, int(glob_id), int(starttime), int(endtime), int(tusec), st, len(pcts), C.byref(tc),
                                                      C.byref(ts), C.byref(mean)))
        return [s.data_value for s in st], tc.value, ts.value, mean.value

    def export_day_stats(self, tusec, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = (capi.ListenerDayStats * n)()
        capi.check(self.L.gys_export_day_stats(self.h, int(tusec), first, n, C.cast(out, C.c_void_p)))
        return out

    def export_svc_hist(self, which, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 16, 2), dtype=np.int64)
        capi.check(self.L.gys_export_svc_hist(self.h, which, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def export_conn_bitmap(self, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 64), dtype=np.uint16)  # rows 0..31: resp_bitmap_v4_, 32..63: resp_bitmap_v6_
        capi.check(self.L.gys_export_conn_bitmap(self.h, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def export_hll(self):
        out = np.zeros(1 << capi.HLL_P, dtype=np.uint8)
        capi.check(self.L.gys_export_hll(self.h, C.c_void_p(out.ctypes.data)))
        return out

    def export_cms(self, which=0):
        out = np.zeros((capi.CMS_D, capi.CMS_W), dtype=np.int64 if which & 1 else np.uint32)
        capi.check(self.L.gys_export_cms(self.h, which, C.c_void_p(out.ctypes.data)))
        return out

    def export_global_hist(self):
        out = capi.HistRec()
        capi.check(self.L.gys_export_global_hist(self.h, C.byref(out)))
        return out

    def export_tdigest(self, first=0, n=None):
        n = self.num_services() - first if n is None else n
        sums = np.zeros((n, capi.TD_NB), dtype=np.int64)
        cnts = np.zeros((n, capi.TD_NB), dtype=np.uint32)
        mm = np.zeros((n, 2), dtype=np.int32)
        capi.check(self.L.gys_export_tdigest(self.h, first, n, C.c_void_p(sums.ctypes.data), C.c_void_p(cnts.ctypes.data), C.c_void_p(mm.ctypes.data)))
        return sums, cnts, mm

    def export_tdigest_pending(self, first=0, n=None):
        """(npend [n], pend [n][CAP]): each row's live prefix sorted ascending, the rest -1 (the buffer itself is unordered)"""
        n = self.num_services() - first if n is None else n
        npend = np.zeros(n, dtype=np.uint32)
        pend = np.zeros((n, self.L.gys_td_pend_cap(self.h)), dtype=np.int32)
        capi.check(self.L.gys_export_tdigest_pending(self.h, first, n, C.c_void_p(npend.ctypes.data), C.c_void_p(pend.ctypes.data)))
        out = np.full_like(pend, -1)
        for i in range(n):
            out[i, :npend[i]] = np.sort(pend[i, :npend[i]])
        return npend, out

    def export_svc_counters(self, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        capi.check(self.L.gys_export_svc_counters(self.h, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def export_svc_hll(self, first=0, n=None):
        n = self.num_services() - first if n is None else n
        out = np.zeros((n, 1 << self.cfg.svc_hll_p), dtype=np.uint8)
        capi.check(self.L.gys_export_svc_hll(self.h, first, n, C.c_void_p(out.ctypes.data)))
        return out

    def resp_queue_pending(self):
        out = C.c_uint64()
        capi.check(self.L.gys_resp_queue_pending(self.h, C.byref(out)))
        return out.value

    def counters(self):
        out = capi.Counters()
        capi.check(self.L.gys_get_counters(self.h, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def huge_counts(self):
        """which way the large keys (more than 16 384 values in one call) of the last response batch went: 'huge' of them in the batch,
        'fallback' of those merged by the one-workgroup kernel; of the batch's last pool round: 'pool_entries', 'tail_values' (values
        >= 16 384 ms put on the tail list, counted on past its capacity) and 'tier_b' (entries the 512-value merge tier handed on)"""
        out = (C.c_uint32 * 8)()
        capi.check(self.L.gys_debug_huge_counts(self.h, out))
        return {"huge": out[0], "fallback": out[1], "pool_entries": out[2], "tail_values": out[3], "tier_b": out[4]}

    # ---------------------------------------------------------------- measurement helpers
    def profile(self, on=True):
        capi.check(self.L.gys_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        capi.check(self.L.gys_profile_reset(self.h))

    def profile_get(self):
        buf = C.create_string_buffer(1024)
        capi.check(self.L.gys_profile_names(self.h, buf, 1024))
        out = {}
        for name in filter(None, buf.value.decode().split(",")):
            ms, n = C.c_double(), C.c_uint64()
            self.L.gys_profile_get(self.h, name.encode(), C.byref(ms), C.byref(n))
            out[name] = (ms.value, n.value)
        return out

    def gen_resp_events(self, d_ev, nevents, seed, first_host, nhosts, svcs_per_host, zipf_milli=0):
        segs = (capi.RespSeg * nhosts)()
        self.order()
        capi.check(self.L.gys_gen_resp_events_dev(self.h, C.c_void_p(d_ev), nevents, seed, first_host, nhosts, svcs_per_host, zipf_milli, segs))
        return segs
