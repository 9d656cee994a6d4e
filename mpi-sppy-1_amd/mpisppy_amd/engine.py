"""Device engine: one rank's ScenarioBatch resident in HBM + the libphgpu calls.

Owns the caller-side device buffers of include/phgpu.h (torch tensors on the rank's
GPU, scenario-fastest ``[k, S]``) and sequences the per-PH-iteration work:

    solve_loop      -> phgpu_solve                     (spopt.py:226-307)
    Compute_Xbar    -> phgpu_ph_reduce + all-reduce    (phbase.py:27-107)
    Update_W + conv -> phgpu_ph_update + all-reduce    (phbase.py:293-343)
    Ebound/Eobj/E1  -> phgpu_expectations + all-reduce (spopt.py:310-439)
    adaptive rho    -> phgpu_ph_residuals + all-reduce + phgpu_norm_rho_update
                                                       (extensions/norm_rho_updater.py:55-143)
    xhat candidates -> phgpu_nonant_stats + SUM / MAX all-reduces, phgpu_nonant_closest
                                                       (extensions/xhatxbar.py, xhatclosest.py,
                                                        cylinders/slam_heuristic.py)
    gradient rho    -> phgpu_grad_cost, phgpu_w_diff + all-reduce, phgpu_rho_ratio_stats +
                       SUM / MAX all-reduces + phgpu_rho_from_stats
                                                       (utils/gradient.py, find_rho.py, wtracker.py,
                                                        extensions/gradient_extension.py)
    fixer           -> phgpu_fixer_step               (extensions/fixer.py:114-304)
    FWPH            -> phgpu_fwph_direction, phgpu_fwph_column, phgpu_fwph_diff over the handle's
                       column store                   (fwph/fwph.py:210-370, 528-547)
    APH             -> phgpu_aph_reduce + all-reduce, phgpu_aph_norms + all-reduce,
                       phgpu_aph_update, phgpu_select_smallest, phgpu_solve_list, phgpu_aph_mark
                                                       (opt/aph.py:151-195, 254-310, 453-496, 602-646)
    gap estimators  -> phgpu_gap_moments + all-reduce  (confidence_intervals/ciutils.py:400-415)

All launches go to torch's current stream; host synchronisation happens only where
the reference needs a host scalar (the convergence test, bounds).
"""
import atexit
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from .comm import Comm


def _dev_T(a, device, dtype=torch.float64):
    """host [S, k] -> device [k, S] contiguous."""
    a = np.asarray(a)
    if a.ndim == 1:
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(device=device, dtype=dtype)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def combine_node_partials(comm, node_buf):
    """Cross-rank sum of the node-indexed x̄ / x̄² partial buffer (phbase.py:83-87)."""
    return comm.allreduce_sum_(node_buf)


# scenarios at least this large (n + m) whose matrix values are the same in every
# scenario run on the shared-matrix streaming path (path 4, include/phgpu.h
# PHGPU_SHARED_MATRIX); smaller ones fit the register / workgroup-resident paths
SHARED_MIN_SIZE = 8192


# Engines still open at interpreter exit are closed by an atexit hook registered when the
# first engine is made -- after torch's own hooks, so it runs before them (LIFO), while the
# HIP runtime (and a profiler's tool library) is still up.  PHEngine.__del__ at interpreter
# teardown could run after them: a rocprofv3 run of bench.py died in it (SIGSEGV after the
# tool's finalisation, profiles/r04/ac/uc_1.log).
_LIVE = weakref.WeakSet()
_ATEXIT = []


def close_all():
    """Close every engine still open (phgpu_destroy after a device synchronise)."""
    for e in list(_LIVE):
        try:
            e.close()
        except Exception:
            pass


def _track(engine):
    if not _ATEXIT:
        atexit.register(close_all)
        _ATEXIT.append(True)
    _LIVE.add(engine)


def matrix_is_shared(batch):
    """True if every scenario of the batch has the same constraint-matrix values."""
    A = batch.A_val
    return A.shape[0] <= 1 or (A.strides[0] == 0) or bool(np.all(A == A[:1]))


class PHEngine:
    def __init__(self, batch, device=None, comm=None, node_names=None, shared=None):
        """``shared``: None = the shared-matrix path when the matrix is the same in every
        scenario and the scenarios are large (SHARED_MIN_SIZE); True / False force it
        (True requires the same matrix)."""
        if not torch.cuda.is_available():
            raise _lib.PhgpuError("PHEngine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _lib.load()
        self.batch = batch
        self.comm = comm or Comm()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._stream_cache = {}
        b = batch
        S, n, m, nn = b.S, b.n, b.m, b.nn
        self.S, self.n, self.m, self.nn = S, n, m, nn
        # global node numbering (identical on all ranks): node_names of the PH object
        names = node_names if node_names is not None else b.node_names
        gid = {nd: i for i, nd in enumerate(names)}
        remap = np.array([gid[nd] for nd in b.node_names], dtype=np.int32)
        node_of = remap[b.node_of]
        self.node_names = list(names)
        self.num_nodes = len(names)
        self.nlen_max = max(1, b.nlen_max)
        h = ctypes.c_void_p()
        rp = np.ascontiguousarray(b.row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(b.col_idx, dtype=np.int32)
        nc = np.ascontiguousarray(b.nonant_col, dtype=np.int32)
        nd = np.ascontiguousarray(b.nonant_depth, dtype=np.int32)
        no = np.ascontiguousarray(b.nonant_off, dtype=np.int32)
        P = lambda a: a.ctypes.data_as(_lib.P_i32)  # noqa: E731
        if shared is None:
            shared = (n + m) >= SHARED_MIN_SIZE and matrix_is_shared(b)
        elif shared and not matrix_is_shared(b):
            raise ValueError("shared=True needs the same matrix values in every scenario")
        self.shared = bool(shared)
        torch.cuda.set_device(self.dev_index)
        _lib.check(self.lib.phgpu_create2(ctypes.byref(h), self.dev_index, S, n, m, b.nnz, P(rp), P(ci),
                                          nn, P(nc), P(nd), P(no), b.depth, self.num_nodes,
                                          self.nlen_max, _lib.SHARED_MATRIX if self.shared else 0),
                   "phgpu_create2")
        self.h = h
        _track(self)
        # library calls of the PH step, by kind (tests assert which path a loop took)
        self.calls = {"ph_reduce": 0, "ph_update_ex": 0, "ph_step_local": 0, "ph_step_defer": 0,
                      "allreduce_xbar": 0, "allreduce_conv_side": 0, "allreduce_conv_main": 0, "xbar_ahead_used": 0,
                      "ph_loop": 0, "ph_residuals": 0, "norm_rho_update": 0, "allreduce_resid": 0,
                      "solve_deferred": 0, "nonant_stats": 0, "nonant_closest": 0, "allreduce_stats_sum": 0,
                      "allreduce_stats_max": 0, "grad_cost": 0, "w_diff": 0, "rho_ratio_stats": 0,
                      "rho_from_stats": 0, "allreduce_wdiff": 0, "allreduce_ratio_sum": 0, "allreduce_ratio_max": 0,
                      "fixer_step": 0, "fixer_totals_host": 0}
        # several ranks: the conv all-reduce on a side stream under the next solve (False: on
        # the launch stream ahead of it -- bench.py --no-conv-overlap, the comparison case)
        self.overlap_conv = True
        dev = self.device
        self.A_val = _dev_T(b.A_val[0] if self.shared else b.A_val, dev)
        self.c = _dev_T(b.c, dev)
        self.lb = _dev_T(b.lb, dev)
        self.ub = _dev_T(b.ub, dev)
        self.rl = _dev_T(b.rl, dev)
        self.ru = _dev_T(b.ru, dev)
        self.q = _dev_T(b.q, dev)
        self.obj_const = _dev_T(b.obj_const, dev)
        self.prob = _dev_T(b.prob, dev)
        self.node_of = _dev_T(node_of, dev, torch.int32)
        self.prob_coeff = _dev_T(b.prob_coeff, dev)
        # caller-owned I/O buffers
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
        self.x = z(n, S)
        self.y = z(max(m, 1), S)
        self.obj = z(S)
        self.bound = z(S)
        self.status = torch.zeros(S, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(S, dtype=torch.int32, device=dev)
        self.W = z(max(nn, 1), S)
        self.rho = z(max(nn, 1), S)
        self.xbar = z(max(nn, 1), S)
        self.node_buf = z(2 * self.num_nodes * self.nlen_max)
        self.conv_buf = z(1)
        self.exp_buf = z(5)
        self.xfix = None
        self.scen_offset = 0      # global index of local scenario 0 (SPOpt sets it; gap_moments)
        self._gap_out = None
        self.pvar = None        # per-nonant probability coefficients (set_nonant_probs)
        self.W_on = 0
        self.prox_on = 0
        # row duals are an optional phgpu_solve output: PH never reads them, so the hot
        # loop leaves them on the device side (set True to have ``y`` filled by solves)
        self.want_duals = False
        # Host-mapped readbacks (phgpu_ph_update_ex writes conv and the last solve's
        # statistics straight into pinned host memory, no copy launches): launch ids of the
        # last solve launch, of the solve whose outputs are current and of a pending
        # speculative one; row_of maps a launch id to the stats row an update wrote for it.
        self._xbar_pending = False   # compute_xbar(lazy=True) left x̄ to the next update
        self._launch_id = self._cur_id = self._spec_id = 0
        self._gripe_id = 0
        self._row_of = {}
        self._stats_rows = torch.zeros((1, 6), dtype=torch.int64).pin_memory()
        self._stats_tmp = torch.zeros(6, dtype=torch.int64).pin_memory()
        # conv readback: the update kernel (one rank) or the copy behind the conv all-reduce
        # (several ranks) stores conv into this pinned word, which the host set to NaN before
        # the update was queued; the host polls it -- no event marker in the PH step (each
        # marker is a barrier packet that idles the GPU ~5.6 us)
        self._conv_host = torch.full((1,), float("nan"), dtype=torch.float64).pin_memory()
        self._conv_np = self._conv_host.numpy()
        self._conv_zero_copy = False
        self._conv_seq = 0        # the update whose conv the pending readback returns
        self._conv_seen = 0       # the last update whose conv (and statistics) the host has seen
        self._side = None         # side stream of the conv all-reduce (several ranks)
        self._ahead_id = 0        # launch whose x xbar_ahead reduced into node_buf (0: none)
        self._conv_ev = None      # the event behind its copy to pinned memory
        self._wait_stats = None   # the pinned statistics row the pending update writes (one rank)
        # markers: the event behind an update (by update number), recorded lazily, only when
        # the host needs an update's statistics before its conv arrived
        self._upd_seq = 0
        self._upd_marks = {}
        self._upload()
        self._native = False
        self._native_comm()

    # -------------------------------------------------------------- plumbing
    def _native_comm(self):
        """The PH step's rank sums through the library's own RCCL communicator (include/phgpu.h
        phgpu_comm_init): ncclAllReduce straight on the engine's stream instead of a
        torch.distributed call (~15 us of host time each in c10d, twice per PH iteration on
        the host's critical path)."""
        plan = getattr(self.comm, "rccl_plan", lambda: None)()
        if plan is None:
            return
        nranks, rank = plan
        # two communicators: the launch stream's x̄ sums (slot 0) and the side stream's conv
        # sums (slot 1), so that neither alternates between streams
        ids = [ctypes.create_string_buffer(128) for _ in range(2)]
        if rank == 0:
            for u in ids:
                _lib.check(self.lib.phgpu_comm_unique_id(u), "phgpu_comm_unique_id")
        raw = [u.raw for u in ids]
        if nranks > 1:
            raw = self.comm.bcast_object(raw if rank == 0 else None, root=0)
        for slot in (0, 1):
            u = ctypes.create_string_buffer(bytes(raw[slot]), 128)
            _lib.check(self.lib.phgpu_comm_init(self.h, u, int(nranks), int(rank), slot), "phgpu_comm_init")
        self._native = True

    def _ar(self, t, tag="critical"):
        """In-place sum of a device fp64 tensor over the ranks (tag "overlapped": the side
        stream's conv sum, on the library's second communicator)."""
        if self._native and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous():
            _lib.check(self.lib.phgpu_allreduce_sum(self.h, 1 if tag == "overlapped" else 0, _ptr(t),
                                                    int(t.numel()), self._stream()), "phgpu_allreduce_sum")
            return self.comm.after_native_(t)
        return self.comm.allreduce_sum_(t)

    def _stream(self):
        # the current stream's handle, cached by the stream's identity (torch's
        # current_stream builds a Stream object per call: ~5 us, twice per PH iteration on
        # the host's critical path)
        key = torch._C._cuda_getCurrentStream(self.dev_index)
        h = self._stream_cache.get(key)
        if h is None:
            h = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._stream_cache[key] = h
        return h

    def _upload(self):
        _lib.check(self.lib.phgpu_set_scenarios(
            self.h, _ptr(self.A_val), _ptr(self.c), _ptr(self.lb), _ptr(self.ub), _ptr(self.rl),
            _ptr(self.ru), _ptr(self.q), _ptr(self.obj_const), _ptr(self.prob), _ptr(self.node_of),
            _ptr(self.prob_coeff), self._stream()), "phgpu_set_scenarios")
        self._bind()

    def _bind(self):
        # (APH binds its own dual weights and prox centre, aph_bind; None: W and x̄)
        W, centre = getattr(self, "_aph_bound", None) or (self.W, self.xbar)
        _lib.check(self.lib.phgpu_set_ph_state(self.h, _ptr(W), _ptr(self.rho), _ptr(centre),
                                               self.W_on, self.prox_on), "phgpu_set_ph_state")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._flush_step()
            torch.cuda.synchronize(self.device)
            if getattr(self, "_side", None) is not None:
                self._side.synchronize()
            self.lib.phgpu_destroy(self.h)
            self.h = None
        _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self):
        return int(self.lib.phgpu_workspace_bytes(self.h))

    def kernel_info(self):
        """Which solve kernel the handle uses (phgpu_kernel_info)."""
        info = (ctypes.c_int32 * 20)()
        _lib.check(self.lib.phgpu_kernel_info(self.h, info), "phgpu_kernel_info")
        keys = ["instance", "lanes", "kc", "zc", "kr", "zr", "KC", "ZC", "KR", "ZR",
                "wg_instance", "wps", "wKC", "wZC", "wKR", "wZR", "path", "rec", "jit_eligible", "jit_wpe"]
        return dict(zip(keys, list(info)))

    def stream_info(self):
        """Path 4 of the last solve (phgpu_stream_info): workgroups per scenario of its
        cluster form (0: the queue), whether the last solve took path 4."""
        info = (ctypes.c_int32 * 2)()
        _lib.check(self.lib.phgpu_stream_info(self.h, info), "phgpu_stream_info")
        return {"cluster": int(info[0]), "path4": int(info[1])}

    def ipm_info(self):
        """Path 6 (interior point) of the handle (phgpu_ipm_info)."""
        info = (ctypes.c_double * 16)()
        _lib.check(self.lib.phgpu_ipm_info(self.h, info), "phgpu_ipm_info")
        keys = ["eligible", "nf_bound", "off", "compiled", "rows", "factor_entries", "scratch_bytes", "compile_s",
                "factor_flops", "solve_flops", "lanes", "folded_steps", "kernel", "jam_handovers", "recentrings",
                "lds_slacks"]
        return dict(zip(keys, list(info)))

    def ipm_prof(self):
        """Per-wave timelines of the last path-6 launch (diagnostics; modules built with
        IPM_PROF in PHGPU_IPM_DEFS on a handle created with PHGPU_IPM_PROF=1): an
        [waves, 16] uint64 array (phgpu_ipm_prof), or None without the buffer."""
        n = int(self.lib.phgpu_ipm_prof(self.h, None, 0))
        if n < 0:
            _lib.check(-1, "phgpu_ipm_prof")
        if n == 0:
            return None
        out = np.zeros(n, dtype=np.uint64)
        rc = int(self.lib.phgpu_ipm_prof(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), n))
        if rc < 0:
            _lib.check(rc, "phgpu_ipm_prof")
        return out.reshape(-1, 16)

    # -------------------------------------------------------------- PH state
    def set_rho(self, rho):
        """rho: scalar, host [nn] array (the same per-nonant rho in every scenario) or host
        [S, nn] array (the rho Params of phbase.py:598-602)."""
        self._flush_step()
        if np.isscalar(rho):
            self.rho.fill_(float(rho))
        elif np.ndim(rho) == 1:
            r = torch.as_tensor(np.asarray(rho, dtype=np.float64), device=self.device)
            assert r.shape[0] == self.nn, (r.shape, self.nn)
            self.rho[:self.nn].copy_(r[:, None].expand(self.nn, self.S))
        else:
            self.rho.copy_(_dev_T(np.asarray(rho, dtype=np.float64), self.device))

    def set_W(self, W):
        self._flush_step()
        self.W.copy_(_dev_T(np.asarray(W, dtype=np.float64), self.device))

    def set_ipm_tuning(self, tuning):
        """Interior-point constants for this handle's modules ({"IPM_SIG_MIN": 0.003, ...};
        phgpu_set_ipm_tuning, before the first solve): a model's measured values."""
        defs = ";".join(f"{k}={v if isinstance(v, int) else repr(float(v))}" for k, v in (tuning or {}).items())
        _lib.check(self.lib.phgpu_set_ipm_tuning(self.h, defs.encode()), "phgpu_set_ipm_tuning")

    def set_nonant_probs(self, var_prob):
        """Per-nonant probability coefficients, host [S, nn] (SPBase.var_prob), or None:
        the x̄ weights and the Update_W mask of variable probabilities (phgpu_set_nonant_probs,
        spbase.py:394-437, phbase.py:315-318)."""
        self._flush_step()
        if var_prob is None:
            self.pvar = None
        else:
            self.pvar = _dev_T(np.asarray(var_prob, dtype=np.float64), self.device)
            assert tuple(self.pvar.shape) == (self.nn, self.S), self.pvar.shape
        _lib.check(self.lib.phgpu_set_nonant_probs(self.h, _ptr(self.pvar)), "phgpu_set_nonant_probs")

    def set_xbar(self, xbar):
        self._flush_step()
        self.xbar.copy_(_dev_T(np.asarray(xbar, dtype=np.float64), self.device))

    def set_terms(self, W_on, prox_on):
        self.W_on = 1 if W_on else 0
        self.prox_on = 1 if prox_on else 0
        self._bind()

    # -------------------------------------------------------------- instrumentation
    _AR_TIMED = 8

    def instrument(self, max_solves, every=1):
        """Record every ``every``-th of the next ``max_solves`` phgpu_solve launches: HIP
        events on the launch stream around the launch and its statistics (status counts,
        iteration sum and maximum; written to pinned memory by the next update kernel, the
        last launch's by phgpu_solve_stats).  Used by bench.py for the per-launch roofline
        inside its timed region; each event is a marker packet that idles the GPU ~5.6 us,
        so the bench samples one step in ``every``."""
        self._ins = {"events": [], "ids": [], "max": int(max_solves), "every": max(1, int(every)), "seen": 0,
                     "ar_events": [], "ar_count": 0,
                     "rows": torch.zeros((max_solves + 4, 6), dtype=torch.int64).pin_memory(), "next": 0}

    def instrumented(self):
        """[(launch ms, scenario-iterations)] of the recorded launches (syncs)."""
        return [(a.elapsed_time(b), int(st[4])) for (a, b), st in self._ins_stats()]

    def instrumented_not_optimal(self):
        """Scenarios not OPTIMAL in each recorded launch."""
        return [int(st[1:4].sum()) for _, st in self._ins_stats()]

    def _ins_stats(self):
        """[(event pair, stats[6])] of the recorded launches whose statistics are known: the
        update after a launch wrote them (phgpu_ph_update_ex), or the launch is the last
        one (phgpu_solve_stats).  Synchronises."""
        ins = getattr(self, "_ins", None)
        if not ins:
            return []
        torch.cuda.synchronize(self.device)
        out = []
        for ev, lid in zip(ins["events"], ins["ids"]):
            st = self._stats_of(lid)
            if st is not None:
                out.append((ev, st))
        return out

    def _recording(self):
        """True while instrumenting (the next ``max_solves`` solves)."""
        ins = getattr(self, "_ins", None)
        return ins is not None and ins["seen"] < ins["max"]

    def _marker(self, seq=None):
        """The event behind update ``seq`` (default: the last one), recorded now if it has
        none yet (then it also covers whatever was queued since)."""
        seq = self._upd_seq if seq is None else seq
        ev = self._upd_marks.get(seq)
        if ev is None:
            ev = torch.cuda.Event()
            ev.record()
            self._upd_marks[seq] = ev
        return ev

    def _stats_of(self, lid):
        """Statistics of launch ``lid`` (host int64[6] copy) or None if no longer known."""
        where = self._row_of.get(lid)
        if where is not None:
            rows, r, seq = where
            if seq > self._conv_seen:   # the update's conv (written after them) not seen yet
                self._marker(seq).synchronize()
            return rows[r].clone()
        if lid == self._launch_id and lid:
            _lib.check(self.lib.phgpu_solve_stats(self.h, _ptr(self._stats_tmp), self._stream()), "phgpu_solve_stats")
            torch.cuda.current_stream(self.device).synchronize()
            return self._stats_tmp.clone()
        return None

    def instrumented_allreduce_ms(self, tag=None):
        """Total ms of the x̄ / conv all-reduces issued while instrumenting (HIP events on
        the issuing stream around each collective; 0 with one rank, where they are no-ops);
        ``tag`` "critical" / "overlapped" selects the x̄ or the conv ones."""
        ins = getattr(self, "_ins", None)
        if not ins:
            return 0.0
        torch.cuda.synchronize(self.device)
        evs = [(ev, t) for ev, t in ins["ar_events"] if tag is None or t == tag]
        if not evs or not ins["ar_events"]:
            return 0.0
        mean = sum(a.elapsed_time(b) for (a, b), _ in evs) / len(evs)
        return float(mean * ins["ar_count"] * len(evs) / len(ins["ar_events"]))

    def _allreduce_sum_(self, t, tag="critical"):
        """comm.allreduce_sum_ with HIP events around it while instrumenting (``tag``:
        "critical", ahead of the next solve on the launch stream, or "overlapped", the conv
        all-reduce on the side stream)."""
        ins = getattr(self, "_ins", None)
        if ins is None or self.comm.size == 1 or not self._recording():
            return self._ar(t, tag)
        # the first _AR_TIMED all-reduces are timed (each event record is a marker packet
        # that idles the GPU ~5.6 us); the rest are counted and the mean extrapolated
        ins["ar_count"] += 1
        if len(ins["ar_events"]) >= self._AR_TIMED:
            return self._ar(t, tag)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        self._ar(t, tag)
        ev[1].record()
        ins["ar_events"].append((ev, tag))
        return t

    # -------------------------------------------------------------- hot path
    _OUTS = ("x", "y", "obj", "bound", "status", "iters")

    def solve(self, options=None, warm=True, speculative=False):
        """phgpu_solve into the output tensors (x, y, obj, bound, status, iters), or with
        ``speculative`` (phgpu_solve_deferred) into a second set that ``commit()`` swaps in
        (PHBase.iterk_loop launches the next solve before it knows whether the convergence
        test stops the loop).  An uncommitted speculative solve changes nothing: its
        outputs stay in the spare set and the library keeps its warm-start state in a
        second slot that only phgpu_commit makes current (include/phgpu.h)."""
        # a pending lazy x̄ is computed now; a deferred PH step stays with the library, which
        # folds it into this launch or runs it ahead of it (phgpu_ph_step_defer)
        if getattr(self, "_xbar_pending", False):
            self.compute_xbar()
        o = options if options is not None else _lib.default_options()
        if speculative:
            if not hasattr(self, "_spec"):
                self._spec = {k: torch.empty_like(getattr(self, k)) for k in self._OUTS}
            out = self._spec
        else:
            out = {k: getattr(self, k) for k in self._OUTS}
        ins = getattr(self, "_ins", None)
        rec = False
        if self._recording():
            rec = ins["seen"] % ins["every"] == 0
            ins["seen"] += 1
        if rec:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            if self._upd_seq and self._upd_marks.get(self._upd_seq) is None:
                self._upd_marks[self._upd_seq] = ev[0]   # the update's marker, shared
        self._launch_id += 1
        if speculative:
            self._spec_id = self._launch_id
            self.calls["solve_deferred"] += 1
        else:
            self._cur_id = self._launch_id
        self._step_deferred = False   # the library folds a deferred step into this launch or runs it first
        fn = self.lib.phgpu_solve_deferred if speculative else self.lib.phgpu_solve
        _lib.check(fn(self.h, ctypes.byref(o), 1 if warm else 0, _ptr(out["x"]),
                      _ptr(out["y"] if self.want_duals else None), _ptr(out["obj"]), _ptr(out["bound"]),
                      _ptr(out["status"]), _ptr(out["iters"]), self._stream()),
                   "phgpu_solve_deferred" if speculative else "phgpu_solve")
        if rec:
            ev[1].record()
            # the launch's statistics come with the next update (phgpu_ph_update_ex), the
            # last launch's from phgpu_solve_stats after the loop: no copy per launch
            ins["events"].append(ev)
            ins["ids"].append(self._launch_id)

    def commit(self):
        """Make the last speculative solve's outputs and warm-start state the current ones."""
        for k in self._OUTS:
            cur = getattr(self, k)
            setattr(self, k, self._spec[k])
            self._spec[k] = cur
        _lib.check(self.lib.phgpu_commit(self.h), "phgpu_commit")
        self._cur_id = self._spec_id

    def _status_counts(self):
        if not hasattr(self, "_counts_dev"):
            self._counts_dev = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._counts_host = torch.zeros(4, dtype=torch.int32).pin_memory()
            self._counts_ev = torch.cuda.Event()
        _lib.check(self.lib.phgpu_status_counts(self.h, _ptr(self.status), _ptr(self._counts_dev), self._stream()),
                   "phgpu_status_counts")

    def count_not_optimal(self):
        """Number of local scenarios whose last solve is not OPTIMAL (phgpu_status_counts,
        one small read back)."""
        self._status_counts()
        c = self._counts_dev.cpu()
        return int(c[1:].sum())

    def count_not_optimal_async(self):
        """The same count for the current solve, without device work now: the next
        ``update`` writes its statistics (accumulated in the path-6 kernels) to pinned host
        memory with the convergence value, so ``pending_not_optimal`` after the next
        convergence readback costs nothing; without an update in between it asks
        phgpu_solve_stats (one small copy and a wait)."""
        self._gripe_id = self._cur_id

    def pending_not_optimal(self):
        st = self._stats_of(self._gripe_id)
        if st is None:  # a later launch replaced the library's statistics: count statuses
            return self.count_not_optimal()
        return int(st[1:4].sum())

    def ph_loop(self, options, max_iters, convthresh):
        """PHBase.iterk_loop of one rank in one launch (phgpu_ph_loop): up to ``max_iters``
        iterations of x̄ -> W -> conv -> (conv < convthresh: stop) -> solve, on the current
        output set, W, x̄ and node_buf.  Returns {"steps", "end", "ipm_iters", "conv",
        "ms"} -- end 0: the iteration limit, 1: converged, 2: a solve handed scenarios to the
        PDHG fallback (solved; the caller goes on step by step) -- or None when the handle's
        state is not one the loop runs (nothing launched)."""
        if self.comm.size != 1:
            return None
        self._flush_step()
        self._xbar_pending = False          # the loop computes x̄ from x itself
        self._ahead_id = 0
        conv = np.zeros(max(1, int(max_iters)), dtype=np.float64)
        out = np.zeros(4, dtype=np.int64)
        self._launch_id += 1
        self._cur_id = self._launch_id
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        rc = self.lib.phgpu_ph_loop(self.h, ctypes.byref(options), int(max_iters), float(convthresh), _ptr(self.x),
                                    _ptr(self.y if self.want_duals else None), _ptr(self.obj), _ptr(self.bound),
                                    _ptr(self.status), _ptr(self.iters), _ptr(self.node_buf),
                                    conv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), self._stream())
        if rc == -3:
            self.ph_loop_declined = _lib.last_error()     # why the state is not one the loop runs
            return None
        _lib.check(rc, "phgpu_ph_loop")
        ev[1].record()
        ev[1].synchronize()
        self.calls["ph_loop"] += 1
        steps = int(out[0])
        return {"steps": steps, "end": int(out[1]), "ipm_iters": int(out[2]), "conv": conv[:steps].tolist(),
                "ms": ev[0].elapsed_time(ev[1])}

    def compute_xbar_partials(self):
        self.calls["ph_reduce"] += 1
        _lib.check(self.lib.phgpu_ph_reduce(self.h, _ptr(self.x), _ptr(self.node_buf), self._stream()),
                   "phgpu_ph_reduce")
        return self.node_buf

    def compute_xbar(self, lazy=False):
        """Local partials + cross-rank sum (phbase.py:27-87); result left in node_buf.
        ``lazy`` (PHBase.Compute_Xbar with one rank): nothing is launched yet -- the next
        ``update`` does x̄ and the update together (phgpu_ph_step_local: one launch fewer
        for two-stage problems); anything that reads node_buf first computes it.  Several
        ranks: nothing to do when ``xbar_ahead`` already reduced the current solve's x."""
        if lazy and self.comm.size == 1:
            self._xbar_pending = True
            return None
        self._xbar_pending = False
        if self._ahead_id and self._ahead_id == self._cur_id:
            self._ahead_id = 0
            self.node_buf, self._node_ahead = self._node_ahead, self.node_buf
            self.calls["xbar_ahead_used"] += 1
            return self.node_buf
        self._ahead_id = 0
        self.compute_xbar_partials()
        if self.comm.size > 1:
            self.calls["allreduce_xbar"] += 1
        self._allreduce_sum_(self.node_buf)
        return self.node_buf

    def xbar_ahead(self):
        """Several ranks (PHBase.iterk_loop): reduce the speculative solve's x and start the x̄
        all-reduce before the convergence test of the current iteration is known, so the next
        iteration's x̄ is on its way when the host returns from the test.  Used by the next
        ``compute_xbar`` if that solve is committed (its buffer then becomes node_buf), dropped
        otherwise; node_buf keeps the x̄ of the last update meanwhile (xbar_by_node after the
        loop), and every rank issues the same collectives in the same order."""
        if self.comm.size == 1 or not hasattr(self, "_spec"):
            return
        if getattr(self, "_node_ahead", None) is None:
            self._node_ahead = torch.zeros_like(self.node_buf)
        self.calls["ph_reduce"] += 1
        _lib.check(self.lib.phgpu_ph_reduce(self.h, _ptr(self._spec["x"]), _ptr(self._node_ahead), self._stream()),
                   "phgpu_ph_reduce")
        self.calls["allreduce_xbar"] += 1
        self._allreduce_sum_(self._node_ahead)
        self._ahead_id = self._spec_id

    def _flush_xbar(self):
        self._flush_step()
        if getattr(self, "_xbar_pending", False):
            self.compute_xbar()

    def _flush_step(self):
        """Run a step phgpu_ph_step_defer still holds (no solve has folded it yet)."""
        if getattr(self, "_step_deferred", False):
            self._step_deferred = False
            _lib.check(self.lib.phgpu_ph_step_flush(self.h), "phgpu_ph_step_flush")

    def update(self, update_W=True, defer=False):
        """Scatter x̄, W += rho (x - x̄), local conv (phbase.py:90-103, 293-339).  One rank:
        conv goes straight to pinned host memory (no copy launch; with several ranks it
        stays on the device for the all-reduce).  The last launch's statistics go to
        pinned host memory in the same kernel (the gripe and the instrumentation read
        them there).  ``defer`` (one rank, x̄ pending: PHBase.iterk_loop's speculative
        step) hands the step to phgpu_ph_step_defer, which folds it into the next solve
        launch when it can; the solve must follow before anything reads W."""
        if self._upd_seq > self._conv_seen and self._conv_zero_copy:
            # the previous update's conv / statistics were never read back: its kernel may
            # still store into the pinned words after the sentinels below are set
            torch.cuda.current_stream(self.device).synchronize()
        self._conv_zero_copy = self.comm.size == 1
        conv = self._conv_host if self._conv_zero_copy else self.conv_buf
        self._conv_np[0] = float("nan")     # the readback's sentinel (before the launch)
        self._upd_seq += 1
        self._upd_marks = {k: v for k, v in self._upd_marks.items() if k > self._upd_seq - 4}
        self._upd_marks[self._upd_seq] = None
        stats = None
        if self._launch_id:
            ins = getattr(self, "_ins", None)
            if ins is not None and ins["next"] < ins["rows"].shape[0]:
                rows, r = ins["rows"], ins["next"]
                ins["next"] += 1
            else:
                rows, r = self._stats_rows, 0
                self._row_of = {k: v for k, v in self._row_of.items() if v[0] is not rows}
            self._row_of[self._launch_id] = (rows, r, self._upd_seq)
            stats = rows[r]
            rows.numpy()[r] = -1            # the statistics' sentinels (convergence_wait)
        self._wait_stats = stats.numpy() if (stats is not None and self._conv_zero_copy) else None
        if getattr(self, "_xbar_pending", False):
            self._xbar_pending = False
            fn = self.lib.phgpu_ph_step_defer if defer else self.lib.phgpu_ph_step_local
            self.calls["ph_step_defer" if defer else "ph_step_local"] += 1
            _lib.check(fn(self.h, _ptr(self.x), _ptr(self.node_buf), _ptr(self.xbar),
                          _ptr(self.W), _ptr(self.rho), 1 if update_W else 0,
                          _ptr(conv), _ptr(stats), self._stream()), "phgpu_ph_step")
            self._step_deferred = bool(defer)
            return
        self.calls["ph_update_ex"] += 1
        _lib.check(self.lib.phgpu_ph_update_ex(self.h, _ptr(self.x), _ptr(self.node_buf), _ptr(self.xbar),
                                               _ptr(self.W), _ptr(self.rho), 1 if update_W else 0,
                                               _ptr(conv), _ptr(stats), self._stream()), "phgpu_ph_update_ex")

    # -------------------------------------------------------------- adaptive rho
    def _resid_bufs(self):
        if getattr(self, "resid", None) is None:
            half = self.num_nodes * self.nlen_max
            self.resid = torch.zeros(4 * half, dtype=torch.float64, device=self.device)
            self.rho_last = torch.zeros(half, dtype=torch.float64, device=self.device)
            self.nr_counts = torch.zeros(4, dtype=torch.int64, device=self.device)
            self._xbar_prev = None
        return self.num_nodes * self.nlen_max

    def residuals(self):
        """The residual sums of NormRhoUpdater and the convergers (phgpu_ph_residuals;
        norm_rho_updater.py:55-104, primal_dual_converger.py:58-110, norm_rho_converger.py:23-29)
        for the current x, x̄ and rho: four node-indexed planes in ``resid`` (summed over the
        ranks: the reference's per-node and ROOT Allreduces in one) and this rank's
        ``rho_last``.  Device work only."""
        self._flush_xbar()
        self._resid_bufs()
        self.calls["ph_residuals"] += 1
        _lib.check(self.lib.phgpu_ph_residuals(self.h, _ptr(self.x), _ptr(self.xbar), _ptr(self.rho),
                                               _ptr(self.resid), _ptr(self.rho_last), self._stream()),
                   "phgpu_ph_residuals")
        if self.comm.size > 1:
            self.calls["allreduce_resid"] += 1
            self._allreduce_sum_(self.resid)
        return self.resid

    def xbar_snapshot(self):
        """Keep the node x̄ of the last update as the previous average of the next rho update
        (NormRhoUpdater._snapshot_avg, norm_rho_updater.py:50-53): a device copy."""
        self._flush_xbar()
        half = self._resid_bufs()
        if self._xbar_prev is None:
            self._xbar_prev = torch.empty(half, dtype=torch.float64, device=self.device)
        self._xbar_prev.copy_(self.node_buf[:half])

    def norm_rho_update(self, params):
        """NormRhoUpdater.miditer's rule on the device (phgpu_norm_rho_update,
        norm_rho_updater.py:128-143) from the planes ``residuals`` left and the x̄ snapshot,
        which is then renewed (:124).  ``params``: _lib.NormRhoParams."""
        if getattr(self, "_xbar_prev", None) is None or getattr(self, "resid", None) is None:
            raise _lib.PhgpuError("norm_rho_update needs residuals() and an earlier xbar_snapshot()")
        self.calls["norm_rho_update"] += 1
        _lib.check(self.lib.phgpu_norm_rho_update(self.h, ctypes.byref(params), _ptr(self.resid),
                                                  _ptr(self.rho_last), _ptr(self.node_buf), _ptr(self._xbar_prev),
                                                  _ptr(self.rho), _ptr(self.nr_counts), self._stream()),
                   "phgpu_norm_rho_update")
        self.xbar_snapshot()

    def norm_rho_counts(self):
        """Local (k, s) entries of the last rho update that took no action / increased /
        decreased / took the converged decrease (one small read back)."""
        return self.nr_counts.cpu().numpy()

    def residual_planes(self):
        """Host [4, num_nodes * nlen_max] copy of the planes of the last ``residuals``."""
        return self.resid.cpu().numpy().reshape(4, -1)

    def node_xbar_flat(self):
        """Host copy of the node x̄ (first half of node_buf), [num_nodes * nlen_max]."""
        self._flush_xbar()
        return self.node_buf[:self.num_nodes * self.nlen_max].cpu().numpy()

    def primal_gap(self):
        """PrimalDualConverger._compute_primal_convergence (primal_dual_converger.py:58-85)."""
        return float(self.residual_planes()[1].sum())

    def dual_gap(self, xbar_prev):
        """PrimalDualConverger._compute_dual_residual (primal_dual_converger.py:87-110);
        ``xbar_prev``: host node x̄ of the previous test (``node_xbar_flat``)."""
        return float((self.residual_planes()[2] * np.abs(self.node_xbar_flat() - xbar_prev)).sum())

    def rho_norm(self):
        """NormRhoConverger._compute_rho_norm (norm_rho_converger.py:23-29)."""
        return float(self.residual_planes()[3].sum())

    # -------------------------------------------------------------- xhat candidates
    def _nonant_arg(self, v):
        v = v.to(device=self.device, dtype=torch.float64).contiguous()
        assert tuple(v.shape) == (max(self.nn, 1), self.S), v.shape
        return v

    def nonant_stats(self, v):
        """Per-node statistics of a nonant array ``v`` (device [nn, S], the layout of W and of a
        spoke's localnonants; phgpu_nonant_stats): a device [4, num_nodes, nlen_max] tensor
        of the pcoef-weighted sums of v and v² (x̄ and x̄², phbase.py:54-87), -min v and max v
        (slam_heuristic.py:57-84), reduced over the ranks by one SUM (planes 0-1) and one MAX
        (planes 2-3) all-reduce.  Entries no scenario of any rank reaches: 0 / -inf."""
        self._flush_step()
        half = self.num_nodes * self.nlen_max
        if getattr(self, "nstats", None) is None:
            self.nstats = torch.empty(4 * half, dtype=torch.float64, device=self.device)
        v = self._nonant_arg(v)
        self.calls["nonant_stats"] += 1
        _lib.check(self.lib.phgpu_nonant_stats(self.h, _ptr(v), _ptr(self.nstats), self._stream()),
                   "phgpu_nonant_stats")
        if self.comm.size > 1:
            self.calls["allreduce_stats_sum"] += 1
            self._ar(self.nstats[:2 * half])
            self.calls["allreduce_stats_max"] += 1
            self.comm.allreduce_max_(self.nstats[2 * half:])
        return self.nstats.view(4, self.num_nodes, self.nlen_max)

    def closest_scenario(self, v, xbar_node, xsqbar_node):
        """The scenario of ``v`` (device [nn, S]) closest to x̄ in truncated z-score
        (phgpu_nonant_closest, xhatclosest.py:37-65; two-stage only): (smallest distance,
        rank, local index), the same on every rank.  ``xbar_node`` / ``xsqbar_node``: device
        [nlen_max] tensors, the reduced planes 0 / 1 of ``nonant_stats`` or the halves of
        node_buf.  Ties within a rank go to the lowest index, between ranks to the highest
        rank (a MAX of -distance, then a MAX of rank-or--1, as the reference's two
        Allreduces).  ``closest_dist`` keeps the local distances (device [S])."""
        self._flush_step()
        if getattr(self, "closest_dist", None) is None:
            self.closest_dist = torch.empty(self.S, dtype=torch.float64, device=self.device)
            self._closest_best = torch.empty(2, dtype=torch.float64, device=self.device)
        v = self._nonant_arg(v)
        xb = xbar_node.to(device=self.device, dtype=torch.float64).contiguous()
        xs = xsqbar_node.to(device=self.device, dtype=torch.float64).contiguous()
        assert xb.numel() >= self.nlen_max and xs.numel() >= self.nlen_max, (xb.shape, xs.shape)
        self.calls["nonant_closest"] += 1
        _lib.check(self.lib.phgpu_nonant_closest(self.h, _ptr(v), _ptr(xb), _ptr(xs), _ptr(self.closest_dist),
                                                 _ptr(self._closest_best), self._stream()), "phgpu_nonant_closest")
        if self.comm.size == 1:
            d, i = self._closest_best.cpu().tolist()
            return d, 0, int(i)
        t = -self._closest_best[:1].clone()
        self.comm.allreduce_max_(t)
        d, i = self._closest_best.cpu().tolist()
        gmin = -float(t.item())
        r = torch.tensor([float(self.comm.rank) if d <= gmin else -1.0], dtype=torch.float64, device=self.device)
        self.comm.allreduce_max_(r)
        win = int(r.item())
        li = torch.tensor([float(i) if win == self.comm.rank else -1.0], dtype=torch.float64, device=self.device)
        self.comm.allreduce_max_(li)
        return gmin, win, int(li.item())

    # -------------------------------------------------------------- gradient rho
    def grad_cost(self, xn):
        """The gradient cost at the nonant values ``xn`` (device [nn, S], the layout of W):
        cost[k, s] = -(c + q xn) of the stored objective (phgpu_grad_cost; Find_Grad.compute_grad,
        gradient.py:65-81, without its solve).  Returns the device [nn, S] tensor ``gcost``."""
        self._flush_step()
        if getattr(self, "gcost", None) is None:
            self.gcost = torch.zeros_like(self.W)
        xn = self._nonant_arg(xn)
        self.calls["grad_cost"] += 1
        _lib.check(self.lib.phgpu_grad_cost(self.h, _ptr(xn), _ptr(self.gcost), self._stream()), "phgpu_grad_cost")
        return self.gcost

    def w_diff(self):
        """WTracker.W_diff (wtracker.py:134-157, phgpu_w_diff): the mean |W - W_prev| over all
        scenarios and nonants of all ranks.  THIS DEPARTS FROM wtracker.py:155-157 with several
        ranks: the reference sums the ranks' own means and divides by n_proc, which depends on
        how the scenarios are split unless every rank holds equally many; here every rank's mean
        is weighted by its share of the scenarios (the same number for an even split).  W_prev
        (owned here; W at the first call, which therefore gives 0 as the reference's
        local_Ws[-1] = local_Ws[0]) renewed in the same pass.  Device work only: every call's
        value is appended to the device history ``w_hist`` (entry 0 is 0), and the returned
        double[2] view ``w_gate`` = {the previous call's value, this one's} is the gate of
        ``find_rho`` -- no copy between calls.  ``w_diff_value`` reads the last one back."""
        self._flush_step()
        if getattr(self, "w_hist", None) is None:
            self.w_hist = torch.zeros(1024, dtype=torch.float64, device=self.device)
            self._w_n = 0
            self._W_prev = self.W.clone()
        self._w_n += 1
        if self._w_n >= self.w_hist.numel():
            self.w_hist = torch.cat([self.w_hist, torch.zeros_like(self.w_hist)])
        cur = self.w_hist[self._w_n:self._w_n + 1]
        self.calls["w_diff"] += 1
        _lib.check(self.lib.phgpu_w_diff(self.h, _ptr(self.W), _ptr(self._W_prev), _ptr(cur), self._stream()),
                   "phgpu_w_diff")
        if self.comm.size > 1:
            # the mean over ALL scenarios: every rank's mean weighted by its share of them.  The
            # reference divides the sum of the ranks' means by n_proc (wtracker.py:155-157), which
            # is the same number when the ranks hold equally many scenarios and depends on the
            # split when they do not
            cur.mul_(float(self.S) / float(self.total_scenarios()))
            self.calls["allreduce_wdiff"] += 1
            self._ar(cur)
        self.w_gate = self.w_hist[self._w_n - 1:self._w_n + 1]
        return self.w_gate

    def w_diff_value(self):
        """Host value of the last ``w_diff`` (one small read back)."""
        return float(self.w_hist[self._w_n].item())

    def w_diff_history(self):
        """Host array of every ``w_diff`` so far, in call order."""
        return self.w_hist[1:self._w_n + 1].cpu().numpy()

    def total_scenarios(self):
        """Scenarios of all ranks (one all-reduce and read back at the first call)."""
        if getattr(self, "_S_total", None) is None:
            t = torch.tensor([float(self.S)], dtype=torch.float64, device=self.device)
            if self.comm.size > 1:
                self.comm.allreduce_sum_(t)
            self._S_total = int(round(t.item()))
        return self._S_total

    def rho_ratio_stats(self, cost, indep_denom=False, rel_bound=1e3):
        """Per nonant, the sum, -min and max over all scenarios of |cost| / denominator
        (phgpu_rho_ratio_stats; Find_Rho.compute_rho, find_rho.py:170-203, up to the order
        statistic) for the current x and x̄: a device [3, num_nodes, nlen_max] tensor, reduced
        over the ranks by one SUM and one MAX all-reduce.  ``indep_denom``: the scenario-
        independent denominator max(1 / rel_bound, sum_s prob_coeff |x - x̄|) of _grad_denom
        (:118-147), which is plane 1 of ``residuals``; else every scenario's own.  Two-stage
        only (PhgpuError rc=-3 otherwise).  Device work only."""
        self._flush_xbar()
        half = self.num_nodes * self.nlen_max
        if getattr(self, "rr_planes", None) is None:
            self.rr_planes = torch.empty(3 * half, dtype=torch.float64, device=self.device)
        cost = self._nonant_arg(cost)
        gden = None
        if indep_denom:
            self.residuals()
            gden = torch.clamp(self.resid[half:2 * half], min=1.0 / float(rel_bound))
        self.gden = gden
        self.calls["rho_ratio_stats"] += 1
        _lib.check(self.lib.phgpu_rho_ratio_stats(self.h, _ptr(cost), _ptr(self.x), _ptr(self.xbar), _ptr(gden),
                                                  _ptr(self.rr_planes), self._stream()), "phgpu_rho_ratio_stats")
        if self.comm.size > 1:
            self.calls["allreduce_ratio_sum"] += 1
            self._ar(self.rr_planes[:half])
            self.calls["allreduce_ratio_max"] += 1
            self.comm.allreduce_max_(self.rr_planes[half:])
        return self.rr_planes.view(3, self.num_nodes, self.nlen_max)

    def find_rho(self, cost, order_stat, indep_denom=False, rel_bound=1e3, gate=None, thr=0.05, applied=None):
        """rho[k, s] = the order statistic ``order_stat`` (0 the min, 0.5 the mean, 1 the max;
        Find_Rho._order_stat, find_rho.py:150-168) of nonant k's ratios |cost| / denominator
        over all scenarios, for every local scenario (``rho_ratio_stats`` +
        phgpu_rho_from_stats).  ``gate``: a device double[2] tensor {previous, current} dual
        metric (``w_diff``'s ``w_gate``), rho being rewritten only if it moved by at most
        ``thr`` relative (gradient_extension.py:65-68), or None: always.  ``applied``: a device
        int32[1] tensor that receives 1 / 0 (default ``rho_applied``).  Device work only."""
        self.rho_ratio_stats(cost, indep_denom, rel_bound)
        if getattr(self, "rho_applied", None) is None:
            self.rho_applied = torch.zeros(1, dtype=torch.int32, device=self.device)
        applied = self.rho_applied if applied is None else applied
        self.calls["rho_from_stats"] += 1
        _lib.check(self.lib.phgpu_rho_from_stats(self.h, _ptr(self.rr_planes), self.total_scenarios(),
                                                 float(order_stat), _ptr(gate), float(thr), _ptr(self.rho),
                                                 _ptr(applied), self._stream()), "phgpu_rho_from_stats")

    def rho_ratio_planes(self):
        """Host [3, num_nodes * nlen_max] copy of the planes of the last ``rho_ratio_stats``."""
        return self.rr_planes.cpu().numpy().reshape(3, -1)

    def convergence_diff(self):
        """phbase.py:330-343: sum over ranks of per-rank means, / n_proc (host float)."""
        self.convergence_diff_async()
        return self.convergence_wait()

    def convergence_mark(self):
        """Mark the update on the launch stream (several ranks): a following
        ``convergence_diff_async`` waits for this point rather than for whatever was queued
        in between, so PHBase.iterk_loop launches the speculative solve right after the mark
        and issues the side-stream conv work behind it -- the host's side-stream calls (event,
        stream switch, all-reduce, copy) no longer delay the solve's launch (a 35 us idle gap
        per PH iteration in the loopback trace)."""
        if self._conv_zero_copy or self.comm.size == 1:
            return
        if not self.overlap_conv:
            # (the comparison case: the conv all-reduce stays ahead of the solve)
            self.convergence_diff_async()
            self._conv_issued = self._upd_seq
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._mark = (self._upd_seq, ev)

    def convergence_diff_async(self):
        """Start the same readback without waiting; ``convergence_wait`` returns it and work
        queued after this call does not delay it.  One rank: the update kernel stores conv
        into pinned memory itself.  Several ranks: the conv all-reduce (phbase.py:341) and
        its copy into pinned memory run on a side stream behind the update (or behind
        ``convergence_mark``), so the next solve launches at once and only the x̄ all-reduce
        stays ahead of it."""
        self._conv_seq = self._upd_seq
        if self._conv_zero_copy or getattr(self, "_conv_issued", 0) == self._upd_seq:
            return
        main = torch.cuda.current_stream(self.device)
        if self._conv_ev is None:
            self._conv_ev = torch.cuda.Event()
        mark = getattr(self, "_mark", None)
        self._mark = None
        if not self.overlap_conv:
            # (the comparison case of the bench: the conv all-reduce ahead of the next solve on
            # the launch stream, as the reference's Allreduce sits in the loop)
            self.calls["allreduce_conv_main"] += 1
            self._allreduce_sum_(self.conv_buf, tag="critical")
            self._conv_host.copy_(self.conv_buf, non_blocking=True)
            self._conv_ev.record(main)
            self._upd_marks[self._upd_seq] = self._conv_ev
            return
        if mark is not None and mark[0] == self._upd_seq:
            ev = mark[1]                           # recorded right after the update
        else:
            ev = torch.cuda.Event()
            ev.record(main)
        self._upd_marks[self._upd_seq] = ev        # (also the update's marker for its stats)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_event(ev)
        self.calls["allreduce_conv_side"] += 1
        with torch.cuda.stream(self._side):
            self._allreduce_sum_(self.conv_buf, tag="overlapped")
            self._conv_host.copy_(self.conv_buf, non_blocking=True)
            # the host waits for this event, not for the word to change: the copy engine may
            # write the 8 bytes piecewise, and a poll caught a half-written value (its top
            # byte still the NaN sentinel's: 9.4e306 as conv on one rank, round-5 2-rank
            # test), which could make ranks disagree on the break and deadlock
            self._conv_ev.record(self._side)

    _SPIN = 200000

    def convergence_wait(self):
        """The pending conv (polls the pinned word; after a long wait it synchronises the
        streams, which also surfaces a device error)."""
        self._flush_step()          # a deferred step no solve has taken yet: run it now
        a = self._conv_np
        if not self._conv_zero_copy:
            # several ranks: the side stream's copy is complete once its event is -- polled
            # (hipEventQuery), not waited on: the blocking wait returned 15-20 us after the
            # copy had finished, on the host's critical path (loopback trace)
            ev, n = self._conv_ev, 0
            while not ev.query():
                n += 1
                if n > self._SPIN:
                    ev.synchronize()
                    break
            self._conv_seen = max(self._conv_seen, self._conv_seq)
            return float(a[0]) / self.comm.size
        st = self._wait_stats
        n = 0
        while a[0] != a[0] or (st is not None and (st == -1).any()):
            n += 1
            if n > self._SPIN:
                torch.cuda.current_stream(self.device).synchronize()
                if self._side is not None:
                    self._side.synchronize()
                break
        self._conv_seen = max(self._conv_seen, self._conv_seq)
        return float(a[0]) / self.comm.size

    def expectations(self):
        """(Eobj, Ebound, E1, Efeas, Eoptimal) summed over ranks (spopt.py:310-439)."""
        _lib.check(self.lib.phgpu_expectations(self.h, _ptr(self.obj), _ptr(self.bound), _ptr(self.status),
                                               _ptr(self.exp_buf), self._stream()), "phgpu_expectations")
        self.comm.allreduce_sum_(self.exp_buf)
        v = self.exp_buf.cpu().numpy()
        return float(v[0]), float(v[1]), float(v[2]), float(v[3]), float(v[4])

    def gap_moments(self, seg_ptr, f_hat, st_hat, f_star=None, st_star=None, s_off=None):
        """Per-segment moments of two solves' objectives (phgpu_gap_moments; ciutils.py:400-415),
        summed over the ranks: host [nseg, 8] rows {sum p, sum p^2, sum p g, sum p g^2, sum p f_hat,
        sum p f_star, scenarios left out, 0} with g = f_hat - f_star.  ``seg_ptr``: nseg + 1
        ascending global scenario indices; ``f_*`` / ``st_*``: device [S] objectives and statuses
        (``f_star`` and ``st_star`` both None: the zhat4xhat form).  ``s_off``: the global index
        of local scenario 0 (default ``self.scen_offset``, which SPOpt sets).  Reading the
        result is the only synchronisation."""
        sp = torch.as_tensor(np.asarray(seg_ptr, dtype=np.int64)).to(self.device) if not torch.is_tensor(seg_ptr) \
            else seg_ptr.to(device=self.device, dtype=torch.int64).contiguous()
        nseg = int(sp.numel()) - 1
        if self._gap_out is None or self._gap_out.shape[0] != nseg:
            self._gap_out = torch.zeros((max(nseg, 1), 8), dtype=torch.float64, device=self.device)
        off = int(self.scen_offset if s_off is None else s_off)
        self.calls["gap_moments"] = self.calls.get("gap_moments", 0) + 1
        _lib.check(self.lib.phgpu_gap_moments(self.h, _ptr(f_hat), _ptr(st_hat), _ptr(f_star), _ptr(st_star),
                                              _ptr(sp), nseg, off, _ptr(self._gap_out), self._stream()),
                   "phgpu_gap_moments")
        self.comm.allreduce_sum_(self._gap_out)
        return self._gap_out.cpu().numpy()

    def fix_nonants(self, xfix):
        """lb = ub = xfix on the nonant columns of every local scenario (device [nn, S]
        tensor, original units) for the next solves; None restores the model bounds
        (spopt.py:557-660 _fix_nonants / _restore_nonants)."""
        # what the Fixer fixed stays fixed (``fixer_step``): its values fill the NaN entries of
        # ``xfix``, and restoring the model bounds restores them for the free entries only
        held = getattr(self, "fixer_fixval", None)
        if xfix is not None:
            self.xfix = xfix.to(device=self.device, dtype=torch.float64).contiguous()
            assert tuple(self.xfix.shape) == (max(self.nn, 1), self.S), self.xfix.shape
            if held is not None:
                self.xfix = torch.where(torch.isnan(self.xfix), held, self.xfix)
        else:
            self.xfix = None
        arg = self.xfix if self.xfix is not None else held
        _lib.check(self.lib.phgpu_fix_nonants(self.h, _ptr(arg), self._stream()), "phgpu_fix_nonants")

    # -------------------------------------------------------------- fixer
    def _fixer_bufs(self):
        if getattr(self, "fixer_fixval", None) is None:
            half = self.num_nodes * self.nlen_max
            shape = (max(self.nn, 1), self.S)
            self.fixer_count = torch.zeros(shape, dtype=torch.int32, device=self.device)
            self.fixer_fixval = torch.full(shape, float("nan"), dtype=torch.float64, device=self.device)
            self.fixer_nfix = torch.zeros(half, dtype=torch.int32, device=self.device)
            self.fixer_totals = torch.zeros(3, dtype=torch.int64, device=self.device)
            # local scenarios of every node entry (the library keeps its own for totals[2]),
            # counted on the host: no device pass, no synchronisation
            nloc = np.zeros(half, dtype=np.int32)
            if self.nn:
                b = self.batch
                node_of = self.node_of.cpu().numpy().reshape(-1, self.S)
                idx = (node_of[np.asarray(b.nonant_depth, dtype=np.int64)] * self.nlen_max
                       + np.asarray(b.nonant_off, dtype=np.int64)[:, None])
                nloc = np.bincount(idx.ravel(), minlength=half).astype(np.int32)
            self.fixer_nloc = torch.as_tensor(nloc, device=self.device)

    def fixer_prepare(self):
        """Allocate the Fixer's state ahead of the first ``fixer_step`` (Fixer.populate calls
        it after Iter0, so that the PH loop's first miditer only enqueues the pass)."""
        self._fixer_bufs()

    def fixer_arg(self, a, dtype):
        """A per-nonant input of ``fixer_step`` as a device [nn] tensor: thresholds (float64)
        or lags (int32; None or a negative value: the reference's None)."""
        if torch.is_tensor(a):
            t = a.to(device=self.device, dtype=dtype).contiguous()
        elif dtype == torch.int32:
            t = torch.tensor([-1 if v is None or int(v) < 0 else int(v) for v in a], dtype=dtype, device=self.device)
        else:
            t = torch.as_tensor(np.asarray(a, dtype=np.float64), device=self.device)
        assert t.numel() == self.nn, (t.shape, self.nn)
        return t

    def fixer_step(self, params, th, nb, lb, ub):
        """Fixer.miditer on the device (phgpu_fixer_step, fixer.py:114-304) for the current
        x̄ and E[x²]: the counters ``fixer_count``, the values ``fixer_fixval`` (device [nn, S],
        NaN = free) and the working bounds of the newly fixed entries; ``fixer_nfix`` (per
        node entry, this call) and ``fixer_totals`` (accumulated).  ``params``:
        _lib.FixerParams; th / nb / lb / ub: ``fixer_arg`` tensors.  Device work only."""
        self._flush_xbar()
        self._fixer_bufs()
        self.calls["fixer_step"] += 1
        _lib.check(self.lib.phgpu_fixer_step(self.h, ctypes.byref(params), _ptr(self.node_buf), _ptr(th), _ptr(nb),
                                             _ptr(lb), _ptr(ub), _ptr(self.fixer_count), _ptr(self.fixer_fixval),
                                             _ptr(self.fixer_nfix), _ptr(self.fixer_totals), self._stream()),
                   "phgpu_fixer_step")

    def fixer_totals_host(self):
        """(entries newly fixed so far, entries fixed on arrival, node entries that fixed only
        part of their local scenarios) -- the one read back of the Fixer."""
        self.calls["fixer_totals_host"] += 1
        if getattr(self, "fixer_totals", None) is None:
            return 0, 0, 0
        t = self.fixer_totals.cpu().tolist()
        return int(t[0]), int(t[1]), int(t[2])

    # -------------------------------------------------------------- FWPH
    def fwph_init(self, max_cols):
        """The FWPH column store and its buffers (phgpu_fwph_init; fwph.py:685-771): ``fw_What``
        (the LP's dual weights, device [nn, S]), ``fw_xq`` ([nn, S]) and ``fw_xqx`` ([n, S],
        the QP point in x's nonant columns, what the x̄ / W step reads), ``fw_gamma``,
        ``fw_dual_bound``, ``fw_ncols`` ([S]) and the pinned ``fw_counts`` (int32[4]: still
        active, Gamma < -stop_check_tol, LP not OPTIMAL)."""
        self._flush_step()
        _lib.check(self.lib.phgpu_fwph_init(self.h, int(max_cols), self._stream()), "phgpu_fwph_init")
        if getattr(self, "fw_What", None) is None:
            z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)  # noqa: E731
            self.fw_What = torch.zeros_like(self.W)
            self.fw_xq = torch.zeros_like(self.W)
            self.fw_xqx = torch.zeros_like(self.x)
            self.fw_gamma = z(self.S)
            self.fw_dual_bound = z(self.S)
            self.fw_diff = z(1)
            self.fw_exp = z(5)
            self.fw_ncols = torch.zeros(self.S, dtype=torch.int32, device=self.device)
            self.fw_counts = torch.zeros(4, dtype=torch.int32).pin_memory()
            self._fw_counts_np = self.fw_counts.numpy()
            self._fw_ev = torch.cuda.Event()
        self.fw_max_cols = int(max_cols)
        self.calls.setdefault("fwph_column", 0)
        self.calls.setdefault("fwph_direction", 0)

    def fwph_load(self, X, f, a=None):
        """Fill every scenario's store with K columns (phgpu_fwph_load): X device [K, nn, S],
        f device [K, S], a device [K, S] or None (all weight on column 0); rho is the engine's."""
        K = int(X.shape[0])
        X = X.to(device=self.device, dtype=torch.float64).contiguous()
        f = f.to(device=self.device, dtype=torch.float64).contiguous()
        assert tuple(X.shape) == (K, max(self.nn, 1), self.S) and tuple(f.shape) == (K, self.S), (X.shape, f.shape)
        if a is not None:
            a = a.to(device=self.device, dtype=torch.float64).contiguous()
            assert tuple(a.shape) == (K, self.S), a.shape
        _lib.check(self.lib.phgpu_fwph_load(self.h, K, _ptr(X), _ptr(f), _ptr(a), _ptr(self.rho), _ptr(self.fw_xq),
                                            _ptr(self.fw_xqx), self._stream()), "phgpu_fwph_load")

    def fwph_export(self):
        """The store on the host (tests, reporting): dict of X [K, nn, S], f, a [K, S], ncols,
        phi, active, nit [S] and xq [nn, S] numpy arrays.  Synchronises."""
        K, S, nn = self.fw_max_cols, self.S, max(self.nn, 1)
        d = {"X": torch.zeros(K, nn, S, dtype=torch.float64, device=self.device),
             "f": torch.zeros(K, S, dtype=torch.float64, device=self.device),
             "a": torch.zeros(K, S, dtype=torch.float64, device=self.device),
             "ncols": torch.zeros(S, dtype=torch.int32, device=self.device),
             "xq": torch.zeros(nn, S, dtype=torch.float64, device=self.device),
             "phi": torch.zeros(S, dtype=torch.float64, device=self.device),
             "active": torch.zeros(S, dtype=torch.int32, device=self.device),
             "nit": torch.zeros(S, dtype=torch.int32, device=self.device)}
        _lib.check(self.lib.phgpu_fwph_export(self.h, *(_ptr(d[k]) for k in ("X", "f", "a", "ncols", "xq", "phi",
                                                                             "active", "nit")), self._stream()),
                   "phgpu_fwph_export")
        return {k: v.cpu().numpy() for k, v in d.items()}

    def fwph_direction(self, t0, alpha):
        """fw_What = W + rho (src - x̄) (phgpu_fwph_direction, fwph.py:227-247).  Device work only."""
        self.calls["fwph_direction"] += 1
        _lib.check(self.lib.phgpu_fwph_direction(self.h, 1 if t0 else 0, float(alpha), _ptr(self.W), _ptr(self.rho),
                                                 _ptr(self.xbar), _ptr(self.fw_What), self._stream()),
                   "phgpu_fwph_direction")

    def fwph_bind(self, on):
        """Bind fw_What (``on``) or W as the solves' dual weights, W on and prox off."""
        self.W_on, self.prox_on = 1, 0
        _lib.check(self.lib.phgpu_set_ph_state(self.h, _ptr(self.fw_What if on else self.W), _ptr(self.rho),
                                               _ptr(self.xbar), 1, 0), "phgpu_set_ph_state")

    def fwph_column(self, params, t0):
        """One column pass over the last solve (phgpu_fwph_column, fwph.py:256-292); the three
        counts go to the pinned ``fw_counts`` (``fwph_counts`` waits for them).  ``params``:
        _lib.FwphParams.  Device work only."""
        self.calls["fwph_column"] += 1
        self._fw_counts_np[:] = -1
        _lib.check(self.lib.phgpu_fwph_column(self.h, ctypes.byref(params), 1 if t0 else 0, _ptr(self.x),
                                              _ptr(self.obj), _ptr(self.bound), _ptr(self.status), _ptr(self.W),
                                              _ptr(self.fw_What), _ptr(self.rho), _ptr(self.xbar), _ptr(self.fw_gamma),
                                              _ptr(self.fw_dual_bound), _ptr(self.fw_ncols), _ptr(self.fw_xq),
                                              _ptr(self.fw_xqx), _ptr(self.fw_counts), self._stream()),
                   "phgpu_fwph_column")
        self._fw_ev.record()

    def fwph_counts(self):
        """(still active, Gamma < -stop_check_tol, LP not OPTIMAL) of the last column pass over
        the local scenarios: a wait for the pass and a read of pinned memory, no copy."""
        self._fw_ev.synchronize()
        c = self._fw_counts_np
        return int(c[0]), int(c[1]), int(c[2])

    def fwph_diff(self):
        """sum_s prob_s sum_k (xq - x̄)^2 with the current (old) x̄, summed over the ranks
        (phgpu_fwph_diff, fwph.py:528-547): a device [1] tensor."""
        _lib.check(self.lib.phgpu_fwph_diff(self.h, _ptr(self.xbar), _ptr(self.fw_diff), self._stream()),
                   "phgpu_fwph_diff")
        if self.comm.size > 1:
            self._ar(self.fw_diff)
        return self.fw_diff

    def fwph_bound(self):
        """sum_s prob_s dual_bound_s over all ranks (fwph.py:519-526), a host float."""
        _lib.check(self.lib.phgpu_expectations(self.h, _ptr(self.fw_dual_bound), _ptr(self.fw_dual_bound),
                                               _ptr(self.status), _ptr(self.fw_exp), self._stream()),
                   "phgpu_expectations")
        self.comm.allreduce_sum_(self.fw_exp)
        return float(self.fw_exp[1].item())

    def fwph_xbar_step(self, update_W):
        """x̄ from the QP points and, with ``update_W``, W += rho (xq - x̄): phgpu_ph_reduce and
        phgpu_ph_update_ex on ``fw_xqx`` in place of x (fwph.py:120-121, 187, 198)."""
        self._flush_xbar()
        self._ahead_id = 0
        self.calls["ph_reduce"] += 1
        _lib.check(self.lib.phgpu_ph_reduce(self.h, _ptr(self.fw_xqx), _ptr(self.node_buf), self._stream()),
                   "phgpu_ph_reduce")
        if self.comm.size > 1:
            self.calls["allreduce_xbar"] += 1
        self._allreduce_sum_(self.node_buf)
        self.calls["ph_update_ex"] += 1
        _lib.check(self.lib.phgpu_ph_update_ex(self.h, _ptr(self.fw_xqx), _ptr(self.node_buf), _ptr(self.xbar),
                                               _ptr(self.W), _ptr(self.rho), 1 if update_W else 0,
                                               _ptr(self.conv_buf), None, self._stream()), "phgpu_ph_update_ex")

    # -------------------------------------------------------------- APH
    def aph_init(self, use_lag=False):
        """The buffers of APH (mpisppy/opt/aph.py) on the device: ``aph_y``, ``aph_z``, ``aph_u``
        ([nn, S]), ``aph_phi`` ([S]), the three node planes ``aph_planes`` (x̄, E[x²], ȳ, each
        laid out like half of node_buf), ``aph_red`` ([6]: tau, phi, the four squared norms of
        the second reduction), the dispatch state ``aph_mask`` / ``aph_list`` (int32 [S]),
        ``aph_k1``, ``aph_last_iter``, ``aph_last_phi`` ([S]), the pinned ``aph_out`` ([4]: sum
        p W², sum p z², theta, sum phi of phgpu_aph_update).  With ``use_lag`` (APHuse_lag) also
        ``aph_W_lag`` / ``aph_z_lag``, every scenario's W and z as of its last dispatch, which
        are then what Update_y and the solves see."""
        self._flush_step()
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)  # noqa: E731
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.device)  # noqa: E731
        nn, S = max(self.nn, 1), self.S
        self.aph_use_lag = bool(use_lag)
        self.aph_y, self.aph_z, self.aph_u = z(nn, S), z(nn, S), z(nn, S)
        self.aph_phi = z(S)
        self.aph_planes = z(3 * self.num_nodes * self.nlen_max)
        self.aph_red = z(6)
        self.aph_mask, self.aph_list = zi(S), zi(S)
        self.aph_k1, self.aph_last_phi = z(S), z(S)
        self.aph_last_iter = zi(S)
        self.aph_W_lag = z(nn, S) if use_lag else None
        self.aph_z_lag = z(nn, S) if use_lag else None
        self.aph_out = torch.zeros(4, dtype=torch.float64).pin_memory()
        self._aph_out_np = self.aph_out.numpy()
        self._aph_red_host = torch.zeros(6, dtype=torch.float64).pin_memory()
        self._aph_ev = torch.cuda.Event()
        self._aph_bound = None
        for k in ("aph_reduce", "aph_norms", "aph_update", "aph_mark", "select_smallest", "solve_list",
                  "allreduce_aph_planes", "allreduce_aph_scalars", "aph_scalars_read"):
            self.calls.setdefault(k, 0)

    def _aph_use(self):
        return (self.aph_W_lag, self.aph_z_lag) if self.aph_use_lag else (self.W, self.aph_z)

    def aph_bind(self, on=True):
        """Bind W and z (their lagged copies under lag) as the solves' dual weights and prox
        centre, until ``aph_bind(False)``; ``xbar`` stays the engine's x̄ tensor, which spokes
        and extensions read."""
        self._aph_bound = self._aph_use() if on else None
        self._bind()

    def aph_reduce(self, first, mask=None):
        """Update_y and the first reduction (phgpu_aph_reduce, aph.py:151-181, 394-408): y of the
        scenarios in ``mask`` (device int32 [S]; None: all) and the ranks' sum of the three
        planes.  Device work only."""
        Wu, zu = self._aph_use()
        self.calls["aph_reduce"] += 1
        _lib.check(self.lib.phgpu_aph_reduce(self.h, 1 if first else 0, _ptr(mask), _ptr(self.x), _ptr(Wu), _ptr(zu),
                                             _ptr(self.rho),
                                             _ptr(self.aph_y), _ptr(self.aph_planes), self._stream()),
                   "phgpu_aph_reduce")
        if self.comm.size > 1:
            self.calls["allreduce_aph_planes"] += 1
        self._allreduce_sum_(self.aph_planes)

    def aph_norms(self, gamma):
        """x̄, u, phi and the second reduction (phgpu_aph_norms, aph.py:254-310): ``aph_red`` =
        the ranks' sums of {tau, phi, p|u|², p|ȳ|², p W², p z²}, the last two being the local
        sums of the previous phgpu_aph_update, as the reference sends them.  Device work only."""
        self.calls["aph_norms"] += 1
        _lib.check(self.lib.phgpu_aph_norms(self.h, float(gamma), _ptr(self.aph_planes), _ptr(self.x),
                                            _ptr(self.aph_y), _ptr(self.W), _ptr(self.aph_z), _ptr(self.xbar),
                                            _ptr(self.aph_u), _ptr(self.aph_phi), _ptr(self.aph_red), self._stream()),
                   "phgpu_aph_norms")
        self.aph_red[4:6].copy_(self.aph_out[0:2], non_blocking=True)
        if self.comm.size > 1:
            self.calls["allreduce_aph_scalars"] += 1
        self._allreduce_sum_(self.aph_red)

    def aph_update(self, first, nu, gamma):
        """theta, W, z and the post-step phi (phgpu_aph_update, aph.py:453-496, 756); its four
        scalars go to the pinned ``aph_out`` (``aph_scalars`` waits for them).  Device work only."""
        self.calls["aph_update"] += 1
        _lib.check(self.lib.phgpu_aph_update(self.h, 1 if first else 0, float(nu), float(gamma), _ptr(self.aph_red),
                                             _ptr(self.aph_planes), _ptr(self.x), _ptr(self.aph_y), _ptr(self.aph_u),
                                             _ptr(self.W), _ptr(self.aph_z), _ptr(self.aph_phi), _ptr(self.aph_out),
                                             self._stream()), "phgpu_aph_update")
        self._aph_red_host.copy_(self.aph_red, non_blocking=True)
        self._aph_ev.record()

    def aph_scalars(self):
        """(sum p W², sum p z², theta, sum phi) of the last aph_update over the local scenarios
        and the reduced ``aph_red`` as a host array: one wait and a read of pinned memory, the
        iteration's one read."""
        self.calls["aph_scalars_read"] += 1
        self._aph_ev.synchronize()
        o = self._aph_out_np
        return (float(o[0]), float(o[1]), float(o[2]), float(o[3])), self._aph_red_host.numpy().copy()

    def aph_mark(self, it, shelf_life, round_robin):
        """The dispatch record of the scenarios in ``aph_mask`` and every scenario's next first
        key (phgpu_aph_mark, aph.py:646, 529-550, 610-611, 626-629).  Device work only."""
        self.calls["aph_mark"] += 1
        _lib.check(self.lib.phgpu_aph_mark(self.h, _ptr(self.aph_mask), int(it), int(shelf_life),
                                           1 if round_robin else 0, _ptr(self.aph_phi), _ptr(self.aph_last_iter),
                                           _ptr(self.aph_last_phi), _ptr(self.aph_k1), _ptr(self.W), _ptr(self.aph_z),
                                           _ptr(self.aph_W_lag), _ptr(self.aph_z_lag), self._stream()),
                   "phgpu_aph_mark")

    def select_smallest(self, k1, k2, count, mask=None, lst=None):
        """Mark the ``count`` local scenarios smallest by (k1[s], k2[s], s) (phgpu_select_smallest):
        ``mask`` int32 [S] of 0 / 1 and ``lst`` int32 [>= count] in ascending s (default: the
        engine's ``aph_mask`` / ``aph_list``).  ``k1`` may be None.  Device work only."""
        mask = self.aph_mask if mask is None else mask
        lst = self.aph_list if lst is None else lst
        self.calls["select_smallest"] = self.calls.get("select_smallest", 0) + 1
        _lib.check(self.lib.phgpu_select_smallest(self.h, _ptr(k1), _ptr(k2), int(count), _ptr(mask), _ptr(lst),
                                                  self._stream()), "phgpu_select_smallest")
        return mask, lst

    def solve_list(self, lst, count, options=None):
        """A warm solve of the ``count`` scenarios in ``lst`` (device int32, ascending) in place
        (phgpu_solve_list): their entries of the output tensors and of the warm-start state
        are replaced, every other scenario's stay.  Returns the library's code for a
        shared-matrix handle (-3), else 0."""
        if getattr(self, "_xbar_pending", False):
            self.compute_xbar()
        o = options if options is not None else _lib.default_options()
        self.calls["solve_list"] = self.calls.get("solve_list", 0) + 1
        rc = self.lib.phgpu_solve_list(self.h, ctypes.byref(o), _ptr(lst), int(count), _ptr(self.x),
                                       _ptr(self.y if self.want_duals else None), _ptr(self.obj), _ptr(self.bound),
                                       _ptr(self.status), _ptr(self.iters), self._stream())
        if rc == -3 and self.shared:
            return rc
        _lib.check(rc, "phgpu_solve_list")
        if count > 0:
            self._launch_id += 1
            self._cur_id = self._launch_id
            self._step_deferred = False
        return 0

    # -------------------------------------------------------------- L-shaped
    def lshaped_init(self, G, max_cuts, s_off, S_total, R, rl, ru, xlb, xub, etalb):
        """The cut store and the master's data (phgpu_lshaped_init; lshaped.py:84-230): host
        arrays R [n_rows, nn], rl, ru, xlb, xub [nn], etalb [G].  Buffers: ``ls_xhat`` [nn, S]
        (the candidate, what ``fix_nonants`` takes), ``ls_eta`` [G], ``ls_cutbuf`` and the pinned
        ``ls_info`` (12 doubles: phgpu_lshaped_append's 5 at 0, phgpu_lshaped_master's 6 at 6)."""
        self._flush_step()
        f8 = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))  # noqa: E731
        nn, G = self.nn, int(G)
        rl, ru = f8(rl, (-1,)), f8(ru, (-1,))
        n_rows = len(rl)
        R = f8(R, (n_rows, nn))
        xlb, xub, etalb = f8(xlb, (nn,)), f8(xub, (nn,)), f8(etalb, (G,))
        hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
        _lib.check(self.lib.phgpu_lshaped_init(self.h, G, int(max_cuts), int(s_off), int(S_total), n_rows, hp(R),
                                               hp(rl), hp(ru), hp(xlb), hp(xub), hp(etalb), self._stream()),
                   "phgpu_lshaped_init")
        self.ls_G, self.ls_max_cuts = G, int(max_cuts)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)  # noqa: E731
        self.ls_xhat = z(max(nn, 1), self.S)
        self.ls_eta = torch.from_numpy(etalb).to(self.device)
        self.ls_cutbuf = z(G * (nn + 2) + 1)
        self.ls_info = torch.zeros(12, dtype=torch.float64).pin_memory()
        self._ls_info_np = self.ls_info.numpy()
        self._ls_ev = torch.cuda.Event()
        for k in ("lshaped_cuts", "lshaped_append", "lshaped_master", "allreduce_cuts"):
            self.calls[k] = 0

    def lshaped_cuts(self):
        """The groups' cut sums of the last (fixed) solve into ``ls_cutbuf``, summed over the
        ranks (phgpu_lshaped_cuts; lshaped.py:477-520).  The solve must have filled ``y``
        (``want_duals``).  Device work only."""
        self.calls["lshaped_cuts"] += 1
        _lib.check(self.lib.phgpu_lshaped_cuts(self.h, _ptr(self.x), _ptr(self.y), _ptr(self.obj), _ptr(self.status),
                                               _ptr(self.ls_cutbuf), self._stream()), "phgpu_lshaped_cuts")
        if self.comm.size > 1:
            self.calls["allreduce_cuts"] += 1
            self._ar(self.ls_cutbuf)

    def lshaped_append(self, tol):
        """Append the cuts that cut off ``ls_eta`` (phgpu_lshaped_append; lshaped.py:540-560);
        its five numbers go to ``ls_info[0:5]``.  Device work only."""
        self.calls["lshaped_append"] += 1
        self._ls_info_np[:5] = np.nan
        _lib.check(self.lib.phgpu_lshaped_append(self.h, _ptr(self.ls_cutbuf), _ptr(self.ls_eta), float(tol),
                                                 ctypes.c_void_p(self.ls_info.data_ptr()), self._stream()),
                   "phgpu_lshaped_append")
        self._ls_ev.record()

    def lshaped_master(self, options=None):
        """Solve the master into ``ls_xhat`` and ``ls_eta`` (phgpu_lshaped_master; lshaped.py:
        600-630); its six numbers go to ``ls_info[6:12]``.  Device work only."""
        self.calls["lshaped_master"] += 1
        self._ls_info_np[6:] = np.nan
        o = options if options is not None else _lib.default_options()
        _lib.check(self.lib.phgpu_lshaped_master(self.h, ctypes.byref(o), _ptr(self.ls_xhat), _ptr(self.ls_eta),
                                                 ctypes.c_void_p(self.ls_info.data_ptr() + 48), self._stream()),
                   "phgpu_lshaped_master")
        self._ls_ev.record()

    def lshaped_read(self):
        """The iteration's one read: a wait for the last append / master and the pinned
        ``ls_info`` as a dict."""
        self._ls_ev.synchronize()
        v = self._ls_info_np
        return {"added": v[0], "Q": v[1], "held": v[2], "not_optimal": v[3], "wanted": v[4], "bound": v[6],
                "status": v[7], "iters": v[8], "pres": v[9], "dres": v[10], "gap": v[11]}

    def lshaped_load(self, group, a, b):
        """Fill the store from host arrays (phgpu_lshaped_load): group [K], a [K, nn], b [K]."""
        group = np.ascontiguousarray(group, dtype=np.int32)
        K = len(group)
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(K, self.nn))
        b = np.ascontiguousarray(b, dtype=np.float64)
        hp = lambda v: ctypes.c_void_p(v.ctypes.data) if v.size else None  # noqa: E731
        _lib.check(self.lib.phgpu_lshaped_load(self.h, K, hp(group), hp(a), hp(b), self._stream()),
                   "phgpu_lshaped_load")

    def lshaped_export(self):
        """The store on the host (phgpu_lshaped_export): (group [K], a [K, nn], b [K])."""
        mc = self.ls_max_cuts
        group = np.zeros(mc, dtype=np.int32)
        a = np.zeros((mc, self.nn))
        b = np.zeros(mc)
        K = np.zeros(1, dtype=np.int32)
        _lib.check(self.lib.phgpu_lshaped_export(self.h, K.ctypes.data_as(_lib.P_i32), ctypes.c_void_p(group.ctypes.data),
                                                 ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data),
                                                 self._stream()), "phgpu_lshaped_export")
        K = int(K[0])
        return group[:K], a[:K], b[:K]

    # -------------------------------------------------------------- extensive form
    def ef_init(self, zlb, zub, cz, qz, ncomp, cmax, tol, qp):
        """The interior point's store and starting iterate (phgpu_ef_init): host
        arrays zlb, zub, cz, qz [nn] and the counts agreed over the ranks.  Buffers: ``ef_sum``
        (the sums a pass gives to the ranks), ``ef_max`` [2], ``ef_z`` [nn] and the pinned
        ``ef_info`` (phgpu_ef_direction's 8 doubles)."""
        self._flush_step()
        nn = self.nn
        f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(nn))  # noqa: E731
        zlb, zub, cz, qz = f8(zlb), f8(zub), f8(cz), f8(qz)
        hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(self.lib.phgpu_ef_init(self.h, hp(zlb), hp(zub), hp(cz), hp(qz), float(ncomp), float(cmax), float(tol),
                                          int(bool(qp)), self._stream()), "phgpu_ef_init")
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)  # noqa: E731
        self.ef_ntri = nn * (nn + 1) // 2
        self.ef_sum = z(self.ef_ntri + 2 * nn + 2)
        self.ef_max = z(2)
        self.ef_z = z(nn)
        self.ef_info = torch.zeros(8, dtype=torch.float64).pin_memory()
        self._ef_info_np = self.ef_info.numpy()
        self._ef_ev = torch.cuda.Event()
        for k in ("ef_schur", "ef_direction", "ef_step", "allreduce_ef"):
            self.calls[k] = 0

    def _ef_ranks(self, nsum, nmax):
        """The ranks' sum of ef_sum[:nsum] and maximum of ef_max[:nmax]."""
        if self.comm.size > 1:
            self.calls["allreduce_ef"] += 1 + (nmax > 0)
            self._ar(self.ef_sum[:nsum] if nsum < self.ef_sum.numel() else self.ef_sum)
            if nmax:
                self.comm.allreduce_max_(self.ef_max)

    def ef_schur(self, stage):
        """The scenario pass of one right-hand side, summed over the local scenarios and the
        ranks (phgpu_ef_schur).  Device work only."""
        self.calls["ef_schur"] += 1
        _lib.check(self.lib.phgpu_ef_schur(self.h, int(stage), _ptr(self.ef_sum), _ptr(self.ef_max), self._stream()),
                   "phgpu_ef_schur")
        self._ef_ranks(self.ef_sum.numel() if stage == 0 else self.nn, 2 if stage == 0 else 0)

    def ef_direction(self, stage):
        """The Schur complement's solve, the direction pass and its reductions over the ranks
        (phgpu_ef_direction); stage 0 stores the iterate's test in ``ef_info``."""
        self.calls["ef_direction"] += 1
        if stage == 0:
            self._ef_info_np[:] = np.nan
        _lib.check(self.lib.phgpu_ef_direction(self.h, int(stage), _ptr(self.ef_sum), _ptr(self.ef_max),
                                               ctypes.c_void_p(self.ef_info.data_ptr()), self._stream()),
                   "phgpu_ef_direction")
        if stage == 0:
            self._ef_ev.record()
        self._ef_ranks(3, 2)

    def ef_step(self, stage):
        """Sigma (stage 0) or the step (stage 1) (phgpu_ef_step).  Device work only."""
        self.calls["ef_step"] += 1
        _lib.check(self.lib.phgpu_ef_step(self.h, int(stage), _ptr(self.ef_sum), _ptr(self.ef_max), self._stream()),
                   "phgpu_ef_step")

    def ef_iteration(self):
        """One predictor-corrector iteration: nothing is read on the host."""
        for stage in (0, 1):
            self.ef_schur(stage)
            self.ef_direction(stage)
            self.ef_step(stage)

    def ef_read(self):
        """The iteration's one read: a wait for the last stage-0 direction call and the pinned
        ``ef_info`` as a dict (the test of the iterate that iteration started from)."""
        self._ef_ev.synchronize()
        v = self._ef_info_np
        return {"iter": v[0], "mu": v[1], "pres": v[2], "dres": v[3], "gap": v[4], "obj": v[5], "done": v[6]}

    def ef_export(self):
        """The iterate into ``x``, ``y``, ``obj``, ``bound``, ``status``, ``iters`` and ``ef_z``
        (phgpu_ef_export)."""
        _lib.check(self.lib.phgpu_ef_export(self.h, _ptr(self.x), _ptr(self.y), _ptr(self.obj), _ptr(self.bound),
                                            _ptr(self.status), _ptr(self.iters), _ptr(self.ef_z), self._stream()),
                   "phgpu_ef_export")

    # -------------------------------------------------------------- multistage extensive form
    def eft_init(self, nlens, node_depth, node_parent, seg_start, zlb, zub, cz, qz, ncomp, cmax, tol, qp):
        """The tree interior point's store and starting iterate (phgpu_eft_init): host
        arrays nlens [D], node_depth, node_parent [Nn], seg_start [G + 1] and zlb, zub, cz, qz [Ztot]
        in node order.  Buffers: ``ef_z`` [Ztot] and the pinned ``ef_info`` of ``ef_read``."""
        self._flush_step()
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        nlens, node_depth, node_parent, seg_start = i4(nlens), i4(node_depth), i4(node_parent), i4(seg_start)
        Ztot = int(nlens[node_depth].sum())
        f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(Ztot))  # noqa: E731
        zlb, zub, cz, qz = f8(zlb), f8(zub), f8(cz), f8(qz)
        hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(self.lib.phgpu_eft_init(self.h, len(nlens), hp(nlens), len(node_depth), hp(node_depth), hp(node_parent),
                                           hp(seg_start), hp(zlb), hp(zub), hp(cz), hp(qz), float(ncomp), float(cmax),
                                           float(tol), int(bool(qp)), self._stream()), "phgpu_eft_init")
        self.eft_nodes, self.eft_ztot = len(node_depth), Ztot
        self.ef_z = torch.zeros(Ztot, dtype=torch.float64, device=self.device)
        self.ef_info = torch.zeros(8, dtype=torch.float64).pin_memory()
        self._ef_info_np = self.ef_info.numpy()
        self._ef_ev = torch.cuda.Event()
        for k in ("eft_schur", "eft_direction", "eft_step"):
            self.calls[k] = 0

    def eft_fix(self, zfix):
        """Hold entries of z at values for the solve that follows (phgpu_eft_fix): host
        ``zfix`` [Ztot] in node order, NaN where the entry stays free.  After ``eft_init``, before the
        first ``eft_schur``."""
        zfix = np.ascontiguousarray(np.asarray(zfix, dtype=np.float64).reshape(self.eft_ztot))
        _lib.check(self.lib.phgpu_eft_fix(self.h, ctypes.c_void_p(zfix.ctypes.data), self._stream()), "phgpu_eft_fix")

    def eft_schur(self, stage, inspect=False):
        """The scenario pass, its sums per deepest node, the elimination up the tree and ROOT's sums
        (phgpu_eft_schur).  Device work only.  ``inspect``: returns device copies (A [Nn, nn, nn]
        lower triangles, b [Nn, nn]) of every node's matrix (stage 0) and right-hand side as summed."""
        self.calls["eft_schur"] += 1
        A = b = None
        if inspect:
            A = torch.zeros(self.eft_nodes, self.nn, self.nn, dtype=torch.float64, device=self.device)
            b = torch.zeros(self.eft_nodes, self.nn, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.phgpu_eft_schur(self.h, int(stage), _ptr(A) if inspect else None, _ptr(b) if inspect else None,
                                            self._stream()), "phgpu_eft_schur")
        return (A, b) if inspect else None

    def eft_direction(self, stage):
        """ROOT's solve, the back-substitution, the direction pass and its sums (phgpu_eft_direction);
        stage 0 stores the iterate's test in ``ef_info``."""
        self.calls["eft_direction"] += 1
        if stage == 0:
            self._ef_info_np[:] = np.nan
        _lib.check(self.lib.phgpu_eft_direction(self.h, int(stage), ctypes.c_void_p(self.ef_info.data_ptr()), self._stream()),
                   "phgpu_eft_direction")
        if stage == 0:
            self._ef_ev.record()

    def eft_step(self, stage):
        """Sigma (stage 0) or the step (stage 1) (phgpu_eft_step).  Device work only."""
        self.calls["eft_step"] += 1
        _lib.check(self.lib.phgpu_eft_step(self.h, int(stage), self._stream()), "phgpu_eft_step")

    def eft_iteration(self):
        """One predictor-corrector iteration on the tree: nothing is read on the host."""
        for stage in (0, 1):
            self.eft_schur(stage)
            self.eft_direction(stage)
            self.eft_step(stage)

    def eft_read(self):
        """The iteration's one read (``ef_read``: the same record)."""
        return self.ef_read()

    def eft_export(self):
        """The iterate into ``x``, ``y``, ``obj``, ``bound``, ``status``, ``iters`` and ``ef_z`` [Ztot]
        (phgpu_eft_export)."""
        _lib.check(self.lib.phgpu_eft_export(self.h, _ptr(self.x), _ptr(self.y), _ptr(self.obj), _ptr(self.bound),
                                             _ptr(self.status), _ptr(self.iters), _ptr(self.ef_z), self._stream()),
                   "phgpu_eft_export")

    # -------------------------------------------------------------- bundles
    def bundle_init(self, seg_start, zlb, zub, ncomp, cmax, tol, ztol, qp):
        """The segmented interior point's store (phgpu_bundle_init): host arrays
        seg_start [G + 1], zlb, zub [G, nn], ncomp, cmax [G]; ``tol``, ``ztol``: the bundles' test.  ``bundle_info`` is the pinned record
        phgpu_bundle_direction stores at stage 0."""
        self._flush_step()
        seg = np.ascontiguousarray(seg_start, dtype=np.int32)
        G = len(seg) - 1
        f8 = lambda a, *s: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(*s))  # noqa: E731
        zlb, zub, ncomp, cmax = f8(zlb, G, self.nn), f8(zub, G, self.nn), f8(ncomp, G), f8(cmax, G)
        hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(self.lib.phgpu_bundle_init(self.h, G, hp(seg), hp(zlb), hp(zub), hp(ncomp), hp(cmax), float(tol),
                                              float(ztol), int(bool(qp)), self._stream()), "phgpu_bundle_init")
        self.bundle_G, self.bundle_seg = G, seg
        self.bundle_nsum0 = self.nn * (self.nn + 1) // 2 + 2 * self.nn + 2
        self.bundle_info = torch.zeros(8, dtype=torch.float64).pin_memory()
        self._bundle_info_np = self.bundle_info.numpy()
        self._bundle_ev = torch.cuda.Event()
        for k in ("bundle_solve", "bundle_schur", "bundle_direction", "bundle_step"):
            self.calls[k] = 0

    def bundle_start(self):
        """A cold start of every bundle from W, rho, x̄ and the W_on / prox_on switches."""
        _lib.check(self.lib.phgpu_bundle_start(self.h, self._stream()), "phgpu_bundle_start")

    def bundle_schur(self, stage, inspect=False):
        """The scenario pass and the segmented reduction (phgpu_bundle_schur).  ``inspect``: device
        copies (rsum [G, nsum0], rmax [G, 2], terms [nsum0 + 2, S]) are returned."""
        self.calls["bundle_schur"] += 1
        out = (None, None, None)
        if inspect:
            z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.device)  # noqa: E731
            out = (z(self.bundle_G, self.bundle_nsum0), z(self.bundle_G, 2), z(self.bundle_nsum0 + 2, self.S))
        _lib.check(self.lib.phgpu_bundle_schur(self.h, int(stage), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), self._stream()),
                   "phgpu_bundle_schur")
        return out

    def bundle_direction(self, stage):
        self.calls["bundle_direction"] += 1
        if stage == 0:
            self._bundle_info_np[:] = np.nan
        _lib.check(self.lib.phgpu_bundle_direction(self.h, int(stage), ctypes.c_void_p(self.bundle_info.data_ptr()),
                                                   self._stream()), "phgpu_bundle_direction")
        if stage == 0:
            self._bundle_ev.record()

    def bundle_step(self, stage):
        self.calls["bundle_step"] += 1
        _lib.check(self.lib.phgpu_bundle_step(self.h, int(stage), self._stream()), "phgpu_bundle_step")

    def bundle_read(self):
        """The iteration's one read: a wait for the last stage-0 direction call and the pinned
        record (the test of the iterates that iteration started from)."""
        self._bundle_ev.synchronize()
        v = self._bundle_info_np
        return {"open": int(v[1]), "pres": float(v[2]), "dres": float(v[3]), "gap": float(v[4]), "stopped": int(v[5]),
                "iter": int(v[6])}

    def bundle_solve(self, max_iter):
        """phgpu_solve's counterpart with bundles: every bundle's extensive form from a cold start
        into x, y, obj, bound, status, iters.  One read of pinned memory per interior-point
        iteration; the loop ends when no bundle is iterating any more, or after ``max_iter``
        iterations with a last test of the iterates.  Returns the last record and ``passes``."""
        if getattr(self, "_xbar_pending", False):
            self.compute_xbar()
        self._flush_step()
        self.calls["bundle_solve"] += 1
        self._launch_id += 1
        self._cur_id = self._launch_id
        self.bundle_start()
        r, passes = None, 0
        for _ in range(int(max_iter)):
            # the whole iteration is queued before the read: the record is stored by the stage-0
            # direction call, and once no bundle iterates every later kernel returns at once
            for stage in (0, 1):
                self.bundle_schur(stage)
                self.bundle_direction(stage)
                self.bundle_step(stage)
            r = self.bundle_read()
            if r["open"] == 0:
                break
            passes += 1
        else:
            self.bundle_schur(0)          # the test of the last iterates (nothing steps)
            self.bundle_direction(0)
            r = self.bundle_read()
        _lib.check(self.lib.phgpu_bundle_export(self.h, _ptr(self.x), _ptr(self.y if self.want_duals else None),
                                                _ptr(self.obj), _ptr(self.bound), _ptr(self.status), _ptr(self.iters),
                                                self._stream()), "phgpu_bundle_export")
        r["passes"] = passes
        return r

    def fix_nonants_by_node(self, table):
        """Fix every local scenario's nonants at per-node values: ``table`` is a device
        [num_nodes, nlen_max] tensor (global node order of ``node_names``); nonant k of
        scenario s gets table[node_of[depth_k, s], off_k] (the per-node cache of
        spopt.py:557-592)."""
        if not hasattr(self, "_fix_index"):
            d = torch.as_tensor(self.batch.nonant_depth, dtype=torch.long, device=self.device)
            o = torch.as_tensor(self.batch.nonant_off, dtype=torch.long, device=self.device)
            self._fix_index = self.node_of.long().index_select(0, d) * self.nlen_max + o[:, None]
        t = table.reshape(-1).to(device=self.device, dtype=torch.float64)
        self.fix_nonants(t[self._fix_index])

    def nonant_x_dev(self):
        """[nn, S] device tensor of the nonant values of the last solve."""
        idx = torch.as_tensor(self.batch.nonant_col, dtype=torch.long, device=self.device)
        return self.x.index_select(0, idx)

    # -------------------------------------------------------------- host views
    def nonant_x(self):
        """[S, nn] host array of the nonant values (W cache 'ci' order, phbase.py:355-365)."""
        idx = torch.as_tensor(self.batch.nonant_col, dtype=torch.long, device=self.device)
        return self.x.index_select(0, idx).T.cpu().numpy()

    def host(self, name):
        self._flush_step()
        if name == "node_buf":
            self._flush_xbar()
        t = getattr(self, name)
        a = t.cpu().numpy()
        return a.T if a.ndim == 2 else a

    def node_xbar(self):
        """{node name: x̄ vector} from the (reduced) node buffer."""
        self._flush_xbar()
        buf = self.node_buf.cpu().numpy()
        nl = self.nlen_max
        return {nd: buf[g * nl:(g + 1) * nl] for g, nd in enumerate(self.node_names)}
