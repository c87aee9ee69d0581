"""Host-side mirror of the reference's hot-path closures, calling the HIP library through its C ABI.

Reference seam (there is no FFI in the reference; the seam is created at these four closures):
  indirect defectCalc    src/multiShoot_CRTBP_indirect.jl:63-90
  indirect jacobianCalc  src/multiShoot_CRTBP_indirect.jl:93-146
  direct   defectCalc    src/multiShoot_CRTBP_direct.jl:66-109
  direct   jacobianCalc  src/multiShoot_CRTBP_direct.jl:111-166  (+ tf partial :503-516)

Names, argument meaning and return shapes follow the Julia closures; arrays are numpy in the reference's
(column-major) shapes, e.g. XC_all is (12, n_nodes).  The Julia glue that binds the same C ABI is
julia/LowThrustOptHIP.jl.  Nothing here computes on the CPU: without the HIP
library and a GPU every call raises.
"""
import collections
import ctypes as C

import weakref

import numpy as np

from . import _lib
from .constants import MU, RK4, RKF78_FIXED, RKF78_ADAPTIVE, DOP853_ADAPTIVE  # noqa: F401
from ._lib import LtoError, LtoIntegrator, LtoParams, LtoDirectParams, LtoDirectTargets, LtoDirectOrbits, LtoDirectEndModel, LtoDirectTfBounds, LTO_EINVAL


def integrator(method=DOP853_ADAPTIVE, steps=0, rtol=1e-13, atol=1e-13, max_steps=0):
    """lto_integrator.  Default = adaptive order-8 pair at reltol = abstol = 1e-13, the reference's
    Vern8 setting (src/multiShoot_CRTBP_indirect.jl:79)."""
    return LtoIntegrator(int(method), int(steps), float(rtol), float(atol), int(max_steps))


def make_params(MU, DU, TU, thrustLimit, mass, time_direction, p, rho):
    """The reference's `params` tuple (src/multiShoot_CRTBP_indirect.jl:260)."""
    return LtoParams(float(MU), float(DU), float(TU), float(thrustLimit), float(mass), float(time_direction), float(p),
                     float(rho))


def _params_array(params):
    if isinstance(params, LtoParams):
        params = [params]
    elif isinstance(params, tuple) and len(params) == 8 and np.isscalar(params[0]):   # the bare 8-tuple
        params = [make_params(*params)]
    params = [p if isinstance(p, LtoParams) else make_params(*p) for p in params]
    arr = (LtoParams * len(params))(*params)
    return arr, len(params)


def _f64(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One lto_ctx = one GPU (one process per GPU)."""

    def __init__(self, device=0):
        self.lib = _lib.load_library()
        h = C.c_void_p()
        rc = self.lib.lto_create(C.byref(h), int(device))
        if rc != 0:
            raise LtoError(rc, "lto_create failed (no gfx950 device visible?)")
        self.handle = h
        self.device = int(device)
        self._plans = weakref.WeakSet()      # device-resident plans created on this context

    def close(self):
        """Plans first, then the context.  (The C library tolerates the other order too -- lto_destroy defers while
        plans are alive -- but a closed Context should not leave live handles behind.)"""
        if getattr(self, "handle", None):
            for pl in list(self._plans):
                pl.close()
            # page-locked blocks stay with their numpy arrays (pinned_empty): each is freed when its last view dies, and
            # the library completes this destroy with the last of them (lto.h: lifetime)
            self.lib.lto_destroy(self.handle)
            self.handle = None

    def pinned_empty(self, shape, order="F"):
        """numpy float64 array in page-locked host memory (lto_host_alloc).  The host-pointer API reads and writes such
        arrays (and contiguous views into them) in place from the GPU: no copy-engine operation per operand.  The
        memory lives as long as the array or any view of it does, also beyond Context.close(): the block is freed when the
        last of them is collected (lto_host_free finds the owning context by itself)."""
        n = int(np.prod(shape))
        ptr = C.c_void_p()
        self.check(self.lib.lto_host_alloc(self.handle, max(n, 1) * 8, C.byref(ptr)))
        buf = (C.c_double * max(n, 1)).from_address(ptr.value)
        weakref.finalize(buf, self.lib.lto_host_free, None, C.c_void_p(ptr.value))
        return np.frombuffer(buf, dtype=np.float64, count=n).reshape(shape, order=order)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            msg = self.lib.lto_last_error(self.handle)
            raise LtoError(rc, msg.decode() if msg else "")

    def fn(self, name):
        """Entry point lto_<name> of this handle type (a Group substitutes lto_group_<name>)."""
        return getattr(self.lib, "lto_" + name)

    def set_timing(self, on):
        self.check(self.lib.lto_set_timing(self.handle, 1 if on else 0))

    def last_kernel_ms(self):
        return float(self.lib.lto_last_kernel_ms(self.handle))

    def last_call_ms(self):
        """Wall time of the last host-pointer call as measured inside the library (entry to return)."""
        return float(self.lib.lto_last_call_ms(self.handle))

    def last_call_order(self):
        """Lane order of the last host-pointer indirect call: 0 natural, 1 global, 2 windowed (lto_last_call_order)."""
        return int(self.lib.lto_last_call_order(self.handle))

    def calibrate_kernels(self):
        """Measure AUTO's cost table (us per round of every RK4 STM family) on this context's device (lto_calibrate_kernels)."""
        self.check(self.lib.lto_calibrate_kernels(self.handle))
        return {nd: self.kernel_round_costs(nd)[0] for nd in (12, 14)}

    def kernel_lane_round_us(self):
        """us per round of 256 x CUs segments (64 steps) of the whole-segment RK4 kernel (LTO_KERNEL_LANE): default or calibrated."""
        return float(self.lib.lto_kernel_lane_round_us(self.handle))

    def kernel_round_costs(self, ndim):
        """([pipeline8, pipeline48 (48 segments per workgroup), per-lane, pipeline48 (44 segments), pipeline32] us per round at 64
        steps, calibrated?) -- what LTO_KERNEL_AUTO chooses by."""
        out = (C.c_double * 5)()
        cal = C.c_int(0)
        self.check(self.lib.lto_kernel_round_costs(self.handle, int(ndim), out, C.byref(cal)))
        return [float(v) for v in out], bool(cal.value)


class Group:
    """Several GPUs behind this one process (lto_group_*): pass as `ctx=` to indirect_defectCalc, indirect_stm,
    direct_defectCalc and direct_jacobian_blocks (and the functions built on them).  The sweep is split into
    contiguous shards, one host thread and one context per entry of `devices` (ids may repeat)."""

    SWEEPS = ("indirect_defect", "indirect_jacobian", "direct_defect", "direct_jacobian")

    def __init__(self, devices):
        self.lib = _lib.load_library()
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.lib.lto_group_create(len(devices), ids, C.byref(h))
        if rc != 0:
            raise LtoError(rc, "lto_group_create failed")
        self.handle = h
        self.devices = [int(d) for d in devices]

    def fn(self, name):
        if name not in self.SWEEPS:
            raise LtoError(-3, "lto_%s has no group form: use a Context" % name)
        return getattr(self.lib, "lto_group_" + name)

    def check(self, rc):
        if rc != 0:
            msg = self.lib.lto_group_last_error(self.handle)
            raise LtoError(rc, msg.decode() if msg else "")

    def __len__(self):
        return int(self.lib.lto_group_size(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lto_group_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def auto_kernel(ndim, method, steps, p, n_segments, n_cus=256, ordered=False):
    """lto_indirect_auto_kernel: the family LTO_KERNEL_AUTO resolves to for an STM sweep of this shape (MI355X cost table), by name.
    A pure function of the library: needs no GPU."""
    k = _lib.load_library().lto_indirect_auto_kernel(int(ndim), int(method), int(steps), float(p), int(n_segments), int(n_cus), 1 if ordered else 0)
    if k < 0:
        raise LtoError(k, "lto_indirect_auto_kernel: invalid shape")
    return IndirectPlan.KERNEL_NAMES[k]


class Comm:
    """lto_comm: RCCL communicator of one rank (one process per GPU).  `uid` = 128 bytes from Comm.unique_id() on one rank,
    handed to every rank by the launcher (torch.distributed broadcast, MPI, a file).  Operands are device pointers
    (torch tensors or ints); the collectives are asynchronous on `stream`."""

    @staticmethod
    def available():
        return bool(_lib.load_library().lto_comm_available())

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = _lib.load_library().lto_comm_unique_id(buf)
        if rc != 0:
            raise LtoError(rc, "lto_comm_unique_id failed (no RCCL in the process?)")
        return buf.raw

    def __init__(self, ctx, world, rank, uid):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        rc = self.lib.lto_comm_create(ctx.handle, int(world), int(rank), C.create_string_buffer(bytes(uid), 128), C.byref(h))
        if rc != 0:
            raise LtoError(rc, "lto_comm_create failed")
        self.handle = h
        self.world, self.rank = int(world), int(rank)

    WINDOW_BYTES = 128

    @classmethod
    def windows(cls, ctx, world, rank, max_count, exchange):
        """The window transport (lto_comm_window_*): device copies into IPC-mapped receive windows, no RCCL, no compute units for
        the payload; also works for ranks that share a device.  `exchange(handle: bytes) -> list of world handles in rank order`
        is the launcher's all-gather of 128-byte blobs (torch.distributed.all_gather_object, MPI, queues)."""
        # Every rank calls exchange() exactly once, whatever happened before it (a rank that skipped the launcher's collective would
        # leave its peers hanging in it): a failed export travels as an empty blob, and then EVERY rank raises.
        self = cls.__new__(cls)
        self.ctx, self.lib = ctx, ctx.lib
        self.handle = None
        self.world, self.rank = int(world), int(rank)
        h = C.c_void_p()
        blob = C.create_string_buffer(cls.WINDOW_BYTES)
        rc = self.lib.lto_comm_window_export(ctx.handle, int(world), int(rank), int(max_count), blob, C.byref(h))
        if rc == 0:
            self.handle = h
        handles = exchange(blob.raw if rc == 0 else b"")
        if rc != 0:
            raise LtoError(rc, "lto_comm_window_export failed")
        if len(handles) != self.world or any(len(b) != cls.WINDOW_BYTES for b in handles):
            self.close()                 # nobody has opened anything yet: every rank sees the same list and raises here
            raise LtoError(-1, "window export failed on a peer (or exchange() did not return the world handles in rank order)")
        try:
            self.check(self.lib.lto_comm_window_open(self.handle, C.create_string_buffer(b"".join(handles), cls.WINDOW_BYTES * self.world)))
        except LtoError as e:
            e.comm = self                # peers may have mapped this rank's window already: the caller closes it after a barrier
            raise
        return self

    def uses_windows(self):
        return bool(self.lib.lto_comm_uses_windows(self.handle))

    def rccl_ranks(self):
        """Ranks RCCL reports for this communicator (ncclCommCount); 0 for a window communicator."""
        n = self.lib.lto_comm_rccl_ranks(self.handle)
        if n < 0:
            raise LtoError(n, "lto_comm_rccl_ranks failed")
        return int(n)

    def check(self, rc):
        if rc != 0:
            msg = self.lib.lto_comm_last_error(self.handle)
            raise LtoError(rc, msg.decode() if msg else "")

    def failed(self, stream=None):
        """True once a wait of this (window) communicator has run out or the ranks have lost step: results are NaN from then on."""
        f = C.c_int(0)
        self.check(self.lib.lto_comm_status(self.handle, stream, C.byref(f)))
        return bool(f.value)

    def set_wait_limit(self, polls):
        self.check(self.lib.lto_comm_set_wait_limit(self.handle, int(polls)))

    def set_kernel_payload(self, nbytes):
        """Window transport: payloads up to `nbytes` per rank go by the push / collect kernels, larger ones by the copy engines."""
        self.check(self.lib.lto_comm_set_kernel_payload(self.handle, int(nbytes)))

    def allgather(self, send, recv, count, stream=None):
        """recv [world][count] <- send [count] of every rank."""
        self.check(self.lib.lto_comm_allgather_dev(self.handle, stream, _dptr(send), _dptr(recv), int(count)))

    def allreduce(self, buf, count, op="sum", stream=None):
        self.check(self.lib.lto_comm_allreduce_dev(self.handle, stream, _dptr(buf), int(count), 0 if op == "sum" else 1))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lto_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _MemberContext(Context):
    """A group member's context as a Context object (owned by the group: close() only forgets it)."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle
        self.device = int(lib.lto_ctx_device(handle))
        self._plans = weakref.WeakSet()

    def close(self):
        for pl in list(self._plans):
            pl.close()
        self.handle = None


class GroupComm:
    """lto_group_comm: the collectives of an lto_group (one host process, several GPUs).  member(k) is member k's Context
    for device-resident plans; allgather / allreduce take one device pointer per member and run on the members' streams."""

    def __init__(self, group):
        self.group, self.lib = group, group.lib
        h = C.c_void_p()
        rc = self.lib.lto_group_comm_create(group.handle, C.byref(h))
        if rc != 0:
            raise LtoError(rc, "lto_group_comm_create failed")
        self.handle = h
        self.n = len(group)
        self.members = [_MemberContext(self.lib, C.c_void_p(self.lib.lto_group_ctx(group.handle, k))) for k in range(self.n)]

    def uses_rccl(self):
        return bool(self.lib.lto_group_comm_uses_rccl(self.handle))

    def member(self, k):
        return self.members[k]

    def stream(self, k):
        return C.c_void_p(self.lib.lto_ctx_stream(self.members[k].handle))

    def check(self, rc):
        if rc != 0:
            msg = self.lib.lto_group_comm_last_error(self.handle)
            raise LtoError(rc, msg.decode() if msg else "")

    def _ptrs(self, bufs):
        return (C.c_void_p * self.n)(*[_dptr(b) for b in bufs])

    def allgather(self, send, recv, count):
        self.check(self.lib.lto_group_comm_allgather_dev(self.handle, self._ptrs(send), self._ptrs(recv), int(count)))

    def allreduce(self, bufs, count, op="sum"):
        self.check(self.lib.lto_group_comm_allreduce_dev(self.handle, self._ptrs(bufs), int(count), 0 if op == "sum" else 1))

    def synchronize(self):
        import torch
        for k in range(self.n):
            torch.cuda.synchronize(self.members[k].device)

    def close(self):
        if getattr(self, "handle", None):
            for m in self.members:
                m.close()
            self.lib.lto_group_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX = {}


def default_context(device=0):
    if device not in _DEFAULT_CTX:
        _DEFAULT_CTX[device] = Context(device)
    return _DEFAULT_CTX[device]


# ------------------------------------------------------------------------------------------------
# Host-pointer operators (numpy in / numpy out; data crosses PCIe inside the call)
# ------------------------------------------------------------------------------------------------

def _batch_dims(XC):
    if XC.ndim == 2:
        return XC.shape[0], XC.shape[1], 1, False
    if XC.ndim == 3:
        return XC.shape[0], XC.shape[1], XC.shape[2], True
    raise ValueError("expected [ndim x n_nodes] or [ndim x n_nodes x n_batch]")


def _check_out(arrays, shapes, what):
    """Caller-supplied output arrays are written in place by the library (by the GPU itself when page-locked): exact shape,
    Fortran order, float64 and writeable, or nothing is touched."""
    for a, sh in zip(arrays, shapes):
        if not isinstance(a, np.ndarray) or a.shape != sh or not a.flags.f_contiguous or a.dtype != np.float64 or not a.flags.writeable:
            raise LtoError(-1, "out arrays must be writeable Fortran-ordered float64 arrays of shapes " + what)


def _tgrids(t, n_nodes, n_batch):
    t = _f64(t)
    if t.ndim == 1:
        if t.shape[0] != n_nodes:
            raise ValueError("t_TU must have n_nodes entries")
        return t, 1
    if t.shape != (n_nodes, n_batch):
        raise ValueError("t_TU must be [n_nodes] or [n_nodes x n_batch]")
    return t, n_batch


def _indirect_args(XC_all, t_TU, params, integ, ctx):
    """The prologue of the indirect wrappers: (ctx, (ndim, n_nodes, n_batch, batched), the library call's leading arguments
    (handle, ndim, n_nodes, n_batch, XC, t, n_tgrids, params, n_params, integrator)).  The pointers keep their arrays alive."""
    ctx = ctx or default_context()
    integ = integ or integrator()
    XC = _f64(XC_all)
    ndim, n, B, batched = _batch_dims(XC)
    t, ntg = _tgrids(t_TU, n, B)
    prm, nprm = _params_array(params)
    return ctx, (ndim, n, B, batched), (ctx.handle, ndim, n, B, _ptr(XC), _ptr(t), ntg, prm, nprm, C.byref(integ))


def indirect_defectCalc(XC_all, t_TU, params, integ=None, ctx=None, out=None):
    """defectCalc of multiShoot_CRTBP_indirect (:63-90): returns (defect[12 x (n-1)], errors[n-1]).
    A trailing batch axis on XC_all sweeps several trajectories (line-search trial points, homotopy levels)
    in one launch; params may then be one tuple or one per trajectory.  out = (defect, errors): Fortran-ordered float64
    arrays of shapes (ndim, n-1, B) and (n-1, B) written in place."""
    ctx, (ndim, n, B, batched), args = _indirect_args(XC_all, t_TU, params, integ, ctx)
    if out is not None:
        defect, errors = out
        _check_out((defect, errors), ((ndim, n - 1, B), (n - 1, B)), "(ndim, n-1, B) and (n-1, B)")
    else:
        defect = np.zeros((ndim, n - 1, B), order="F")
        errors = np.zeros((n - 1, B), order="F")
    ctx.check(ctx.fn("indirect_defect")(*args, _ptr(defect), _ptr(errors)))
    if not batched:
        return defect[:, :, 0], errors[:, 0]
    return defect, errors


def indirect_stm(XC_all, t_TU, params, integ=None, ctx=None, out=None):
    """Compact Jacobian blocks: Phi[12 x 12 x (n-1)] with Phi[:,:,i] = d x(t_{i+1}) / d XC_all[:,i]
    (the ForwardDiff.jacobian(f, x0) of :121), plus the defect.  out = (Phi, defect): Fortran-ordered float64 arrays of
    shapes (ndim, ndim, n-1, B) and (ndim, n-1, B) written in place (e.g. from Context.pinned_empty)."""
    ctx, (ndim, n, B, batched), args = _indirect_args(XC_all, t_TU, params, integ, ctx)
    if out is not None:
        Phi, defect = out
        _check_out((Phi, defect), ((ndim, ndim, n - 1, B), (ndim, n - 1, B)), "(ndim, ndim, n-1, B) and (ndim, n-1, B)")
    else:
        Phi = np.empty((ndim, ndim, n - 1, B), order="F")
        defect = np.empty((ndim, n - 1, B), order="F")
    ctx.check(ctx.fn("indirect_jacobian")(*args, _ptr(Phi), _ptr(defect)))
    if not batched:
        return Phi[:, :, :, 0], defect[:, :, 0]
    return Phi, defect


def _band(Phi, sparse):
    """Row block i = [Phi_i | -I] at the columns of nodes i and i+1 (jacobianCalc, :123-142), nothing pinned yet: a dense
    array, or a COO matrix that keeps Phi's zeros as stored entries."""
    nd, _, S = Phi.shape
    n = S + 1
    if sparse:
        import scipy.sparse as sp
        rows = (np.arange(S)[:, None, None] * nd + np.arange(nd)[None, :, None] + np.zeros((1, 1, nd), int)).ravel()
        cols = (np.arange(S)[:, None, None] * nd + np.zeros((1, nd, 1), int) + np.arange(nd)[None, None, :]).ravel()
        vals = np.transpose(Phi, (2, 0, 1)).ravel()
        ir = (np.arange(S)[:, None] * nd + np.arange(nd)[None, :]).ravel()
        ic = ir + nd
        return sp.coo_matrix((np.concatenate([vals, -np.ones(S * nd)]),
                              (np.concatenate([rows, ir]), np.concatenate([cols, ic]))), shape=(nd * S, nd * n))
    J = np.zeros((nd * S, nd * n))
    for i in range(S):
        J[nd * i:nd * (i + 1), nd * i:nd * (i + 1)] = Phi[:, :, i]
        J[nd * i:nd * (i + 1), nd * (i + 1):nd * (i + 2)] = -np.eye(nd)
    return J


def indirect_scatter(Phi, sparse=False):
    """Band scatter of jacobianCalc (:123-142): row block i = [Phi_i | -I] at columns 12(i-1)+(1:24)
    (1-based), then columns 1:6 and (end-11):(end-6) zeroed (fixed end states)."""
    nd = Phi.shape[0]
    ns = nd // 2
    J = _band(Phi, sparse)
    if sparse:
        J = J.tolil()
    ncol = J.shape[1]
    J[:, 0:ns] = 0.0
    J[:, ncol - nd:ncol - ns] = 0.0
    return J.tocsc() if sparse else J


def indirect_scatter_mass(Phi, sparse=False):
    """Jac_full of the 14-dim variable-mass system: row block i = [Phi_i | -I] at columns 14 i + (0:28) (0-based), as for
    12 rows, with the pinned columns zeroed -- the first node's r0, v0, m0 (columns 0:7) and the last node's rf, vf and
    lambda_m(tf) (columns 14(n-1) + 0:6 and 14(n-1) + 13).  The final mass, column 14(n-1) + 6, is free."""
    nd = Phi.shape[0]
    if nd != 14:
        raise ValueError("indirect_scatter_mass takes 14 x 14 blocks; got %d rows" % nd)
    J = _band(Phi, sparse)
    last = J.shape[1] - nd
    pinned = np.r_[np.arange(7), last + np.arange(6), last + 13]
    if sparse:
        import scipy.sparse as sp
        keep = np.ones(J.shape[1])
        keep[pinned] = 0.0
        return (J.tocsc() @ sp.diags(keep)).tocsc()
    J[:, pinned] = 0.0
    return J


def indirect_jacobianCalc(XC_all, t_TU, params, integ=None, ctx=None, sparse=False):
    """jacobianCalc of multiShoot_CRTBP_indirect (:93-146): Jac_full [12(n-1) x 12n]."""
    Phi, _ = indirect_stm(XC_all, t_TU, params, integ, ctx)
    return indirect_scatter(Phi, sparse=sparse)


def indirect_newton_step(XC_all, t_TU, params, integ=None, ctx=None, soc_threshold=1e-1, flag_adjointsOnly=False):
    """One Newton iteration on the device (jacobianCalc + least-squares step of optimizeTraj_OLS incl. the
    adjoints-only column mask + second-order correction, indirect.jl:290-296): returns (xc_update, defect)."""
    ctx, (ndim, n, B, batched), args = _indirect_args(XC_all, t_TU, params, integ, ctx)
    upd = np.zeros((ndim, n, B), order="F")
    defect = np.zeros((ndim, n - 1, B), order="F")
    ctx.check(ctx.fn("indirect_newton_step")(*args, 1 if flag_adjointsOnly else 0, float(soc_threshold), _ptr(upd), _ptr(defect)))
    if not batched:
        return upd[:, :, 0], defect[:, :, 0]
    return upd, defect


def indirect_solve(XC_all, t_TU, params, integ=None, flag_adjointsOnly=False, maxIter=10, ctx=None):
    """The Newton loop of multiShoot_CRTBP_indirect (indirect.jl:254-345) as ONE library call, trajectory resident on
    the device: returns (XC_all, defect, status_flag, iterCount, history[k] = (max|defect|, alpha) of iteration k+1).
    indirect_solve_batch with one trajectory."""
    if np.ndim(XC_all) != 2:
        raise ValueError("indirect_solve takes one trajectory [ndim x n_nodes]; indirect_solve_batch takes a batch")
    XC_out, defect, status, iters, history = indirect_solve_batch(XC_all, t_TU, params, integ, flag_adjointsOnly, maxIter, ctx)
    return XC_out[:, :, 0], defect[:, :, 0], int(status[0]), int(iters[0]), history[0]


def indirect_solve_batch(XC_all, t_TU, params, integ=None, flag_adjointsOnly=False, maxIter=10, ctx=None):
    """n_batch independent Newton loops side by side (lto_indirect_solve_batch): XC_all [ndim x n x B] (12 or 14 rows), t_TU [n] or
    [n x B], params one tuple or B.  Returns (XC_all, defect, status_flag[B], iterCount[B], history) with
    history[b] = array of (max|defect|, alpha) per completed iteration of trajectory b."""
    ctx, (ndim, n, B, _), args = _indirect_args(XC_all, t_TU, params, integ, ctx)
    XC_out = np.zeros((ndim, n, B), order="F")
    defect = np.zeros((ndim, n - 1, B), order="F")
    mi = max(int(maxIter), 1)
    hist = np.full((2, mi, B), np.nan, order="F")
    status = np.zeros(B, dtype=np.int32)
    iters = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("indirect_solve_batch")(*args, 1 if flag_adjointsOnly else 0, int(maxIter), _ptr(XC_out), _ptr(defect),
                                             _ptr(status), _ptr(iters), _ptr(hist) if maxIter > 0 else None))
    history = [hist[:, ~np.isnan(hist[1, :, b]), b].T.copy() for b in range(B)]
    return XC_out, defect, status, iters, history


def densify(XC_all, t_TU, params, n_desired, integ=None, ctx=None):
    """densify (src/HelperFunctions.jl:51-101): (XC_dense[ndim x n_desired], t_dense[n_desired]); every segment is
    re-propagated on the GPU and sampled at the uniformly spaced t_dense points that fall inside it.  This is the 12-row entry:
    14-row input (the variable-mass system) is refused here with LtoError -3 and goes to densify_mass."""
    ctx = ctx or default_context()
    integ = integ or integrator()
    XC = _f64(XC_all)
    t = _f64(t_TU)
    ndim, n = XC.shape
    prm, _ = _params_array(params)
    XC_dense = np.zeros((ndim, int(n_desired)), order="F")
    t_dense = np.zeros(int(n_desired))
    ctx.check(ctx.fn("indirect_densify")(ctx.handle, ndim, n, _ptr(XC), _ptr(t), prm, C.byref(integ), int(n_desired),
                                           _ptr(XC_dense), _ptr(t_dense)))
    return XC_dense, t_dense


def densify_mass(XC_all, t_TU, params, n_desired, integ=None, ctx=None):
    """densify for one solution of the 14-row variable-mass system (lto_indirect_densify_mass): XC_all [14 x n],
    params with Isp in the mass slot; (XC_dense [14 x n_desired], t_dense [n_desired]), row 6 the propagated mass.  LTO_RK4 or
    LTO_DOP853_ADAPTIVE."""
    XC = _f64(XC_all)
    if XC.ndim != 2 or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n]")
    t = _f64(t_TU)
    n = XC.shape[1]
    if t.shape != (n,):
        raise ValueError("t_TU must hold one time per node")
    ctx = ctx or default_context()
    integ = integ or integrator()
    prm, _ = _params_array(params)
    XC_dense = np.zeros((14, int(n_desired)), order="F")
    t_dense = np.zeros(int(n_desired))
    ctx.check(ctx.fn("indirect_densify_mass")(ctx.handle, n, _ptr(XC), _ptr(t), prm, C.byref(integ), int(n_desired),
                                                _ptr(XC_dense), _ptr(t_dense)))
    return XC_dense, t_dense


class ThrustEvents:
    """Result of indirect_events; B trajectories (batched) or one (the batch axis dropped): n_events [B], t_event and kind
    [max_events x B], on0 [B], dv [B] (DU/TU), burn_time [B] (TU), dv_seg [(n-1) x B], status [B].  From indirect_events_mass
    also propellant [B] and dm_seg [(n-1) x B] in kg (None otherwise)."""

    def __init__(self, n_events, t_event, kind, on0, dv, burn_time, dv_seg, status, propellant=None, dm_seg=None):
        self.n_events, self.t_event, self.kind, self.on0 = n_events, t_event, kind, on0
        self.dv, self.burn_time, self.dv_seg, self.status = dv, burn_time, dv_seg, status
        self.propellant, self.dm_seg = propellant, dm_seg


def indirect_events(XC_all, t_TU, params, max_events=64, integ=None, ctx=None, with_dv_seg=True):
    """Switch times, burn arcs and dv of indirect solutions (lto_indirect_events_batch): XC_all [12 x n] or
    [12 x n x B], t_TU [n] or [n x B], params one tuple or one per trajectory.  Events are located while the segments are
    integrated (LTO_RK4 or LTO_DOP853_ADAPTIVE); dv is carried as a quadrature state.  Returns a ThrustEvents."""
    XC = _f64(XC_all)
    ndim, n, B, batched = _batch_dims(XC)
    t, ntg = _tgrids(t_TU, n, B)
    prm, nprm = _params_array(params)
    if nprm != 1 and nprm != B:
        raise ValueError("params must be one tuple or one per trajectory")
    M = int(max_events)
    Mr = max(M, 1)
    n_events = np.zeros(B, dtype=np.int32)
    t_event = np.full((Mr, B), np.nan, order="F")
    kind = np.zeros((Mr, B), dtype=np.int32, order="F")
    on0 = np.zeros(B, dtype=np.int32)
    dv, burn = np.zeros(B), np.zeros(B)
    dv_seg = np.zeros((n - 1, B), order="F") if with_dv_seg else None
    status = np.zeros(B, dtype=np.int32)
    ctx = ctx or default_context()
    integ = integ or integrator()
    ctx.check(ctx.fn("indirect_events_batch")(ctx.handle, ndim, n, B, _ptr(XC), _ptr(t), ntg, prm, nprm, C.byref(integ), M,
                                              _ptr(n_events), _ptr(t_event), _ptr(kind), _ptr(on0), _ptr(dv), _ptr(burn),
                                              _ptr(dv_seg), _ptr(status)))
    if not batched:
        return ThrustEvents(int(n_events[0]), t_event[:, 0], kind[:, 0], int(on0[0]), float(dv[0]), float(burn[0]),
                            None if dv_seg is None else dv_seg[:, 0], int(status[0]))
    return ThrustEvents(n_events, t_event, kind, on0, dv, burn, dv_seg, status)


def indirect_events_mass(XC_all, t_TU, params, max_events=64, integ=None, ctx=None, with_dv_seg=True, with_dm_seg=True):
    """indirect_events for the 14-row variable-mass system (lto_indirect_events_mass_batch): XC_all [14 x n] or
    [14 x n x B], params with Isp in the mass slot.  The threshold of p > 1 follows the state's mass.  Returns a ThrustEvents
    with propellant [B] and dm_seg [(n-1) x B] (kg) added."""
    XC = _f64(XC_all)
    if XC.ndim not in (2, 3) or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n] or [14 x n x B]")
    ndim, n, B, batched = _batch_dims(XC)
    t, ntg = _tgrids(t_TU, n, B)
    prm, nprm = _params_array(params)
    if nprm != 1 and nprm != B:
        raise ValueError("params must be one tuple or one per trajectory")
    if not all(prm[k].mass > 0.0 for k in range(nprm)):
        raise ValueError("Isp (the mass slot of 14-row params) must be positive")
    M = int(max_events)
    Mr = max(M, 1)
    n_events = np.zeros(B, dtype=np.int32)
    t_event = np.full((Mr, B), np.nan, order="F")
    kind = np.zeros((Mr, B), dtype=np.int32, order="F")
    on0 = np.zeros(B, dtype=np.int32)
    dv, burn, prop = np.zeros(B), np.zeros(B), np.zeros(B)
    dv_seg = np.zeros((n - 1, B), order="F") if with_dv_seg else None
    dm_seg = np.zeros((n - 1, B), order="F") if with_dm_seg else None
    status = np.zeros(B, dtype=np.int32)
    ctx = ctx or default_context()
    integ = integ or integrator()
    ctx.check(ctx.fn("indirect_events_mass_batch")(ctx.handle, n, B, _ptr(XC), _ptr(t), ntg, prm, nprm, C.byref(integ), M,
                                                   _ptr(n_events), _ptr(t_event), _ptr(kind), _ptr(on0), _ptr(dv), _ptr(burn),
                                                   _ptr(dv_seg), _ptr(prop), _ptr(dm_seg), _ptr(status)))
    if not batched:
        return ThrustEvents(int(n_events[0]), t_event[:, 0], kind[:, 0], int(on0[0]), float(dv[0]), float(burn[0]),
                            None if dv_seg is None else dv_seg[:, 0], int(status[0]), float(prop[0]),
                            None if dm_seg is None else dm_seg[:, 0])
    return ThrustEvents(n_events, t_event, kind, on0, dv, burn, dv_seg, status, prop, dm_seg)


class ControlReplay:
    """Result of control_replay; B starts (batched) or one (the batch axis dropped): x_final [nstate x B], dv [B] (DU/TU),
    accepted / rejected [B] (steps summed over the knot intervals), status [B] (0 ok, 2 no result: NaN), samples
    [nstate x n_samples x B] at the knots sample_knots (None without sampling)."""

    def __init__(self, x_final, dv, accepted, rejected, status, samples, sample_knots):
        self.x_final, self.dv, self.accepted, self.rejected, self.status = x_final, dv, accepted, rejected, status
        self.samples, self.sample_knots = samples, sample_knots


def replay_sample_knots(n_knots, sample_every):
    """The knots control_replay samples: k % sample_every == 0, and the last one; none for sample_every = 0."""
    if sample_every <= 0:
        return np.zeros(0, dtype=np.int64)
    ks = list(range(0, int(n_knots), int(sample_every)))
    if ks[-1] != n_knots - 1:
        ks.append(n_knots - 1)
    return np.array(ks, dtype=np.int64)


def control_replay(x0, lamv, t0, t1, params, integ=None, sample_every=0, ctx=None):
    """Fly a history of lambda_v from many starts (lto_control_replay_batch): x0 [nstate] or [nstate x B] with nstate 6
    (r, v; params.mass the constant mass) or 7 (r, v, m; the mass slot carries Isp); lamv [3 x n_knots] (one history for every
    start) or [3 x n_knots x B] (one per start) at the knots LinRange(t0, t1, n_knots); params one tuple or one per start.  The
    control is the natural cubic spline of lamv, integrated knot interval by knot interval with LTO_RK4 (`steps` per interval) or
    LTO_DOP853_ADAPTIVE.  Returns a ControlReplay."""
    X = _f64(x0)
    if X.ndim not in (1, 2):
        raise ValueError("x0 must be [nstate] or [nstate x B]")
    batched = X.ndim == 2
    X2 = np.asfortranarray(X.reshape(X.shape[0], -1, order="F"))
    nstate, B = X2.shape
    L = _f64(lamv)
    if L.ndim not in (2, 3) or L.shape[0] != 3:
        raise ValueError("lamv must be [3 x n_knots] or [3 x n_knots x n_hist]")
    L3 = np.asfortranarray(L.reshape(3, L.shape[1], -1, order="F"))
    n_knots, n_hist = L3.shape[1], L3.shape[2]
    if n_hist != 1 and n_hist != B:
        raise ValueError("lamv must hold one history or one per start")
    if isinstance(params, tuple) and len(params) == 8 and np.isscalar(params[0]):
        params = make_params(*params)
    prm, nprm = _params_array(params)
    if nprm != 1 and nprm != B:
        raise ValueError("params must be one tuple or one per start")
    every = int(sample_every)
    knots = replay_sample_knots(n_knots, every)
    x_final = np.zeros((nstate, B), order="F")
    samples = np.zeros((nstate, len(knots), B), order="F") if every > 0 else None
    dv = np.zeros(B)
    acc, rej, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    ctx = ctx or default_context()
    integ = integ or integrator()
    ctx.check(ctx.fn("control_replay_batch")(ctx.handle, nstate, n_knots, B, float(t0), float(t1), _ptr(L3), n_hist, _ptr(X2), prm,
                                             nprm, C.byref(integ), every, _ptr(x_final), _ptr(samples), _ptr(dv), _ptr(acc),
                                             _ptr(rej), _ptr(status)))
    if not batched:
        return ControlReplay(x_final[:, 0], float(dv[0]), int(acc[0]), int(rej[0]), int(status[0]),
                             None if samples is None else samples[:, :, 0], knots)
    return ControlReplay(x_final, dv, acc, rej, status, samples, knots)


class GuidanceGains:
    """Result of guidance_gains; B trajectories (batched) or one (the batch axis dropped): K [6 x 6 x (n-1) x B] with
    d lambda_k = K[:, :, k] d x_k, pivot [(n-1) x B] (smallest |u_ii| over the largest |entry| of the matrix solved at that node),
    status [B] (0 ok, 2 not finite, 3 a pivot ratio below sing_tol: K is NaN from that node down to node 0)."""

    def __init__(self, K, pivot, status):
        self.K, self.pivot, self.status = K, pivot, status


def guidance_gains(XC_all, t_TU, params, integ=None, sing_tol=1e-10, ctx=None):
    """Neighbouring-extremal feedback gains of 12-row solutions (lto_guidance_gains_batch): XC_all [12 x n] or
    [12 x n x B], t_TU [n] or [n x B], params one tuple or one per trajectory.  The segment STMs are swept on the device (LTO_RK4 or
    LTO_DOP853_ADAPTIVE) and turned into gains by the backward recurrence that keeps the linearised arrival state fixed.  14-row
    input is refused (LtoError -3).  Returns a GuidanceGains."""
    ctx, (ndim, n, B, batched), args = _indirect_args(XC_all, t_TU, params, integ, ctx)
    S = max(n - 1, 0)
    K = np.zeros((6, 6, S, B), order="F")
    pivot = np.zeros((S, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("guidance_gains_batch")(*args, float(sing_tol), _ptr(K), _ptr(pivot), _ptr(status)))
    if not batched:
        return GuidanceGains(K[:, :, :, 0], pivot[:, 0], int(status[0]))
    return GuidanceGains(K, pivot, status)


class GuidedFlight:
    """Result of guided_flight; B starts (batched) or one (the batch axis dropped): x_final and lam_final [6 x B], dv [B] (DU/TU),
    nodes [6 x n x B] (the state at every node; None unless asked for), accepted / rejected [B] (steps summed over the node
    intervals), status [B] (0 ok, 2 no result: NaN)."""

    def __init__(self, x_final, lam_final, dv, nodes, accepted, rejected, status):
        self.x_final, self.lam_final, self.dv, self.nodes = x_final, lam_final, dv, nodes
        self.accepted, self.rejected, self.status = accepted, rejected, status


def guided_updates(n_nodes, update_every):
    """Number of updates of a guided flight: the nodes k <= n_nodes - 2 with k % update_every == 0; none for update_every = 0."""
    n, every = int(n_nodes), int(update_every)
    if every < 0:
        raise ValueError("update_every must be >= 0")
    return (n - 2) // every + 1 if every > 0 and n >= 2 else 0


def guided_flight(XC_nom, t_TU, K, x0, params, update_every=1, nav=None, integ=None, with_nodes=False, ctx=None):
    """Fly starts under neighbouring-extremal feedback about a nominal (lto_guided_flight_batch): XC_nom [12 x n] with
    t_TU [n] and K [6 x 6 x (n-1)] (one nominal for every start) or [12 x n x B], [n x B], [6 x 6 x (n-1) x B] (one per start); x0 [6]
    or [6 x B]; nav [6 x n_upd] / [6 x n_upd x B] or None, n_upd = guided_updates(n, update_every): the navigation error added to
    the measured state at update j; params one tuple or one per start.  At node k with k % update_every == 0 the costate is reset
    to lambda_nom,k + K_k (x - x_nom,k + e_j); update_every = 0 never updates.  Returns a GuidedFlight."""
    return _guided_flight(6, XC_nom, t_TU, K, x0, params, update_every, nav, integ, with_nodes, ctx)


def _guided_flight(nx, XC_nom, t_TU, K, x0, params, update_every, nav, integ, with_nodes, ctx):
    """guided_flight (nx = 6: ndim as XC_nom has it, the library answers) and guided_flight_mass (nx = 7: XC_nom has 14 rows)."""
    X = _f64(x0)
    if X.ndim not in (1, 2) or X.shape[0] != nx:
        raise ValueError("x0 must be [%d] or [%d x B]" % (nx, nx))
    batched = X.ndim == 2
    X2 = np.asfortranarray(X.reshape(nx, -1, order="F"))
    B = X2.shape[1]
    XC = _f64(XC_nom)
    if XC.ndim not in (2, 3) or (nx == 7 and XC.shape[0] != 14):
        raise ValueError("XC_nom must be [ndim x n] or [ndim x n x n_nom]" if nx == 6 else "XC_nom must be [14 x n] or [14 x n x n_nom]")
    XC3 = np.asfortranarray(XC.reshape(XC.shape[0], XC.shape[1], -1, order="F"))
    ndim, n, n_nom = XC3.shape
    if n_nom != 1 and n_nom != B:
        raise ValueError("XC_nom must hold one nominal or one per start")
    t = _f64(t_TU)
    if t.size != n * n_nom or t.shape[0] != n:
        raise ValueError("t_TU must be [n] or [n x n_nom]")
    t = np.asfortranarray(t.reshape(n, n_nom, order="F"))
    Kg = _f64(K)
    if Kg.size != nx * nx * max(n - 1, 0) * n_nom or Kg.shape[:2] != (nx, nx):
        raise ValueError("K must be [%d x %d x (n-1)] or [%d x %d x (n-1) x n_nom]" % (nx, nx, nx, nx))
    Kg = np.asfortranarray(Kg.reshape(nx, nx, n - 1, n_nom, order="F"))
    every = int(update_every)
    n_upd = guided_updates(n, every)
    E = None
    if nav is not None and n_upd > 0:
        E = _f64(nav)
        if E.shape[0] != nx or E.size != nx * n_upd * B:
            raise ValueError("nav must be [%d x n_upd x B] with n_upd = %d" % (nx, n_upd))
        E = np.asfortranarray(E.reshape(nx, n_upd, B, order="F"))
    prm, nprm = _params_array(params)
    if nprm != 1 and nprm != B:
        raise ValueError("params must be one tuple or one per start")
    if nx == 7 and not all(prm[k].mass > 0.0 for k in range(nprm)):
        raise ValueError("Isp (the mass slot of 14-row params) must be positive")
    x_final, lam_final = np.zeros((nx, B), order="F"), np.zeros((nx, B), order="F")
    dv = np.zeros(B)
    nodes = np.zeros((nx, n, B), order="F") if with_nodes else None
    acc, rej, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    ctx = ctx or default_context()
    integ = integ or integrator()
    tail = (n, B, _ptr(XC3), _ptr(t), _ptr(Kg), n_nom, _ptr(X2), every, _ptr(E), prm, nprm, C.byref(integ), _ptr(x_final),
            _ptr(lam_final), _ptr(dv), _ptr(nodes), _ptr(acc), _ptr(rej), _ptr(status))
    if nx == 6:
        ctx.check(ctx.fn("guided_flight_batch")(ctx.handle, ndim, *tail))
    else:
        ctx.check(ctx.fn("guided_flight_mass_batch")(ctx.handle, *tail))
    if not batched:
        return GuidedFlight(x_final[:, 0], lam_final[:, 0], float(dv[0]), None if nodes is None else nodes[:, :, 0], int(acc[0]),
                            int(rej[0]), int(status[0]))
    return GuidedFlight(x_final, lam_final, dv, nodes, acc, rej, status)


def guidance_gains_mass(XC_all, t_TU, params, integ=None, sing_tol=1e-10, ctx=None):
    """guidance_gains for solutions of the 14-row variable-mass system (lto_guidance_gains_mass_batch): XC_all [14 x n]
    or [14 x n x B], params with Isp in the mass slot.  The gains keep d r_f = d v_f = 0 and d lambda_m(t_f) = 0, the final mass is
    free.  Returns a GuidanceGains with K [7 x 7 x (n-1) x B]: d lambda_k = K[:, :, k] d x_k, x = (r, v, m)."""
    XC = _f64(XC_all)
    if XC.ndim not in (2, 3) or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n] or [14 x n x B]")
    prm, nprm = _params_array(params)
    if not all(prm[k].mass > 0.0 for k in range(nprm)):
        raise ValueError("Isp (the mass slot of 14-row params) must be positive")
    ctx, (ndim, n, B, batched), args = _indirect_args(XC, t_TU, params, integ, ctx)
    S = max(n - 1, 0)
    K = np.zeros((7, 7, S, B), order="F")
    pivot = np.zeros((S, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("guidance_gains_mass_batch")(args[0], *args[2:], float(sing_tol), _ptr(K), _ptr(pivot), _ptr(status)))
    if not batched:
        return GuidanceGains(K[:, :, :, 0], pivot[:, 0], int(status[0]))
    return GuidanceGains(K, pivot, status)


def guided_flight_mass(XC_nom, t_TU, K, x0, params, update_every=1, nav=None, integ=None, with_nodes=False, ctx=None):
    """guided_flight for the 14-row variable-mass system (lto_guided_flight_mass_batch): XC_nom [14 x n (x B)], K
    [7 x 7 x (n-1) (x B)], x0 [7] or [7 x B] (r, v, m), nav [7 x n_upd (x B)] or None, params with Isp in the mass slot.  The update
    resets all seven costates from the seven measured states, the mass included.  Returns a GuidedFlight with x_final and
    lam_final [7 x B] (x_final[6] the final mass) and nodes [7 x n x B]."""
    return _guided_flight(7, XC_nom, t_TU, K, x0, params, update_every, nav, integ, with_nodes, ctx)


GuidanceCovariance = collections.namedtuple("GuidanceCovariance", "P_final P_nodes cov_status K pivot gain_status Phi")


def _covariance_cases(P0, R, update_every, nx):
    """(P0 [nx x nx x n_cases], R likewise, update_every int32 [n_cases], single): the case list of guidance_covariance checked
    before the library is touched; a single [nx x nx] P0 with a scalar update_every is one case."""
    P, Rm = _f64(P0), _f64(R)
    for name, A in (("P0", P), ("R", Rm)):
        if A.ndim not in (2, 3) or A.shape[0] != nx or A.shape[1] != nx:
            raise ValueError("%s must be [%d x %d] or [%d x %d x n_cases]" % (name, nx, nx, nx, nx))
    if P.shape != Rm.shape:
        raise ValueError("P0 and R must have the same shape")
    ev = np.asarray(update_every)
    if ev.ndim > 1 or not np.issubdtype(ev.dtype, np.integer):
        raise ValueError("update_every must be an integer or a vector of integers")
    single = P.ndim == 2 and ev.ndim == 0
    P3 = np.asfortranarray(P.reshape(nx, nx, -1, order="F"))
    R3 = np.asfortranarray(Rm.reshape(nx, nx, -1, order="F"))
    ev = np.ascontiguousarray(ev.reshape(-1), dtype=np.int32)
    n_cases = P3.shape[2]
    if n_cases < 1 or ev.shape[0] != n_cases:
        raise ValueError("update_every must hold one entry per case (%d)" % n_cases)
    if np.any(ev < 0):
        raise ValueError("update_every must be >= 0")
    return P3, R3, ev, single


def guidance_covariance(XC_all, t_TU, params, P0, R, update_every, integ=None, sing_tol=1e-10, with_nodes=False, with_phi=False,
                        ctx=None):
    """Linear covariance of the guided flight about 12-row or 14-row solutions (lto_guidance_covariance_batch):
    XC_all [ndim x n] or [ndim x n x B], ndim 12 or 14 (nx = ndim / 2; 14 rows: params with Isp in the mass slot), t_TU [n] or
    [n x B]; the cases P0, R [nx x nx x n_cases] and update_every [n_cases] (or one [nx x nx] pair with a scalar update_every) are
    shared by all trajectories.  One call sweeps the STMs, builds the gains and runs the forward pass of every (trajectory, case).
    Returns a GuidanceCovariance: P_final [nx x nx x n_cases x B], P_nodes [nx x nx x n x n_cases x B] (with_nodes, else None),
    cov_status [n_cases x B] (0 ok, 2 not finite), K, pivot and gain_status as guidance_gains has them, Phi [ndim x ndim x (n-1) x B]
    (with_phi, else None).  A single case drops the case axis, a single trajectory the batch axis."""
    XC = _f64(XC_all)
    if XC.ndim not in (2, 3) or XC.shape[0] not in (12, 14):
        raise ValueError("XC_all must be [12 x n], [14 x n] or either with a trailing batch axis")
    nx = XC.shape[0] // 2
    P3, R3, ev, single = _covariance_cases(P0, R, update_every, nx)
    prm, nprm = _params_array(params)
    if nx == 7 and not all(prm[k].mass > 0.0 for k in range(nprm)):
        raise ValueError("Isp (the mass slot of 14-row params) must be positive")
    ctx, (ndim, n, B, batched), args = _indirect_args(XC, t_TU, params, integ, ctx)
    if n < 2:
        raise ValueError("XC_all must hold at least two nodes")
    S, nc = n - 1, P3.shape[2]
    K = np.zeros((nx, nx, S, B), order="F")
    pivot = np.zeros((S, B), order="F")
    gain_status = np.zeros(B, dtype=np.int32)
    Phi = np.zeros((ndim, ndim, S, B), order="F") if with_phi else None
    P_nodes = np.zeros((nx, nx, n, nc, B), order="F") if with_nodes else None
    P_final = np.zeros((nx, nx, nc, B), order="F")
    cov_status = np.zeros((nc, B), dtype=np.int32, order="F")
    ctx.check(ctx.fn("guidance_covariance_batch")(*args, float(sing_tol), nc, _ptr(P3), _ptr(R3), _ptr(ev), _ptr(K), _ptr(pivot),
                                                  _ptr(gain_status), _ptr(Phi), _ptr(P_nodes), _ptr(P_final), _ptr(cov_status)))
    if single:
        P_final, cov_status = P_final[:, :, 0], cov_status[0]
        P_nodes = None if P_nodes is None else P_nodes[:, :, :, 0]
    if not batched:
        return GuidanceCovariance(P_final[..., 0], None if P_nodes is None else P_nodes[..., 0],
                                  int(cov_status[0]) if single else cov_status[..., 0], K[:, :, :, 0], pivot[:, 0],
                                  int(gain_status[0]), None if Phi is None else Phi[:, :, :, 0])
    return GuidanceCovariance(P_final, P_nodes, cov_status, K, pivot, gain_status, Phi)


def direct_defectCalc(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, ctx=None):
    """defectCalc of multiShoot_CRTBP_direct (:66-109): returns (defect[nstate x (n-1)], errors[n-1])."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    defect = np.zeros((ns, n - 1, B), order="F")
    errors = np.zeros((n - 1, B), order="F")
    ctx.check(ctx.fn("direct_defect")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm),
                                        _ptr(defect), _ptr(errors)))
    if not batched:
        return defect[:, :, 0], errors[:, 0]
    return defect, errors


def direct_midpoints(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, ctx=None):
    """The propagation of meshRefine_direct (direct.jl:645-656) for every segment at once: returns
    (x_mid[nstate x (n-1)], defect, errors) with x_mid[:, i] = state at the middle of segment i propagated from node i
    with u_i.  nsteps = 2 is the reference's single `ode7` step."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    x_mid = np.zeros((ns, n - 1, B), order="F")
    defect = np.zeros((ns, n - 1, B), order="F")
    errors = np.zeros((n - 1, B), order="F")
    ctx.check(ctx.fn("direct_midpoints")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm),
                                           _ptr(x_mid), _ptr(defect), _ptr(errors)))
    if not batched:
        return x_mid[:, :, 0], defect[:, :, 0], errors[:, 0]
    return x_mid, defect, errors


DirectRefine = collections.namedtuple("DirectRefine", "X U t n n_removed passes status errors")


def direct_refine(X, U, t, nsteps, MU, DU, TU, Isp, tol_min, tol_max, max_nodes, ctx=None):
    """Errors-driven mesh refinement of the direct transcription on the device (lto_direct_refine_batch):
    meshRefine_direct for X [nstate x n] or [nstate x n x B], U [3 x n (x B)], t [n] or [n x B] in ONE library call -- nodes are
    removed while the smallest RKF7(8) estimate is below tol_min, then segments are bisected while the largest is above tol_max
    and the mesh has fewer than max_nodes nodes.  Returns DirectRefine(X [nstate x n'], U [3 x n'], t [n'], n = n', n_removed,
    passes, status (0 refined, 1 stopped at max_nodes, 2 a NaN estimate), errors [n' - 1] of the final mesh), or a list of
    them, one per trajectory, for a batched input (the node counts differ)."""
    X = _f64(X)
    U = _f64(U)
    ns, n, B, batched = _batch_dims(X)
    if ns not in (6, 7):
        raise ValueError("direct_refine: X must have 6 or 7 rows; got shape %s" % (X.shape,))
    if n < 2:
        raise ValueError("direct_refine: need at least two nodes")
    if U.shape != ((3, n, B) if batched else (3, n)):
        raise ValueError("direct_refine: U must be [3 x n_nodes] or [3 x n_nodes x n_batch], as X; got shape %s" % (U.shape,))
    tt, ntg = _tgrids(t, n, B)
    nsteps, M = int(nsteps), int(max_nodes)
    if nsteps < 2:
        raise LtoError(-1, "direct_refine: nsteps must be >= 2")
    if M < n:
        raise LtoError(-1, "direct_refine: max_nodes is the capacity of the result: it must be >= n_nodes")
    tol_min, tol_max = float(tol_min), float(tol_max)
    if np.isnan(tol_min) or np.isnan(tol_max):
        raise LtoError(-1, "direct_refine: a tolerance is NaN")
    ctx = ctx or default_context()
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    Xo = np.empty((ns, M, B), order="F")
    Uo = np.empty((3, M, B), order="F")
    to = np.empty((M, B), order="F")
    eo = np.empty((M - 1, B), order="F")
    n_out, n_rem, passes, status = (np.zeros(B, dtype=np.int32) for _ in range(4))
    ctx.check(ctx.fn("direct_refine_batch")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(tt), ntg, nsteps, C.byref(prm), tol_min,
                                            tol_max, M, _ptr(Xo), _ptr(Uo), _ptr(to), _ptr(n_out), _ptr(n_rem), _ptr(passes),
                                            _ptr(status), _ptr(eo)))
    out = []
    for b in range(B):
        k = int(n_out[b])
        out.append(DirectRefine(np.asfortranarray(Xo[:, :k, b]), np.asfortranarray(Uo[:, :k, b]), to[:k, b].copy(), k, int(n_rem[b]),
                                int(passes[b]), int(status[b]), eo[:k - 1, b].copy()))
    return out if batched else out[0]


DirectResample = collections.namedtuple("DirectResample", "X U t errors_before errors_after status")


def _ragged_slab(parts):
    """The results of direct_refine's batch form side by side: (X [ns x cap x B], U, t [cap x B], n_in [B]), NaN behind every
    trajectory's own nodes -- the layout lto_direct_refine_batch writes."""
    cap, B, ns = max(p.n for p in parts), len(parts), parts[0].X.shape[0]
    X = np.full((ns, cap, B), np.nan, order="F")
    U = np.full((3, cap, B), np.nan, order="F")
    t = np.full((cap, B), np.nan, order="F")
    for b, p in enumerate(parts):
        X[:, :p.n, b], U[:, :p.n, b], t[:p.n, b] = p.X, p.U, p.t
    return X, U, t, np.array([p.n for p in parts], dtype=np.int32)


def direct_resample(X, U=None, t=None, nsteps=10, MU=None, DU=None, TU=None, Isp=None, n_new=None, n_in=None, weights=None,
                    w_floor=0.1, passes=1, ctx=None):
    """Direct solutions resampled onto one node count n_new on the device (lto_direct_resample_batch): the new grid
    equidistributes the RKF7(8) estimates of lto_direct_defect at `nsteps` (weight e^(1/8), floored at w_floor times the largest),
    the new nodes lie on the transcription's own half-arcs.  X [nstate x n_cap (x B)], U [3 x n_cap (x B)], t [n_cap] or
    [n_cap x B]; n_in [B] = the valid columns of every trajectory (None: all), the rest is never read.  X may instead be what
    direct_refine returns -- one DirectRefine or the batch form's list -- with U and t left out.  weights [(n_cap-1) (x B)]
    replace the monitor (passes must be 1).  Returns DirectResample(X [nstate x n_new (x B)], U, t [n_new (x B)], errors_before
    [(n_cap-1) (x B)] (NaN behind the valid part), errors_after [(n_new-1) (x B)], status: 0, 1 the new times were not strictly
    increasing, 2 a NaN estimate; the outputs of such a trajectory are NaN)."""
    if isinstance(X, DirectRefine) or (isinstance(X, (list, tuple)) and len(X) and isinstance(X[0], DirectRefine)):
        if U is not None or t is not None or n_in is not None:
            raise ValueError("direct_resample: a direct_refine result brings its own U, t and node counts")
        batched = not isinstance(X, DirectRefine)
        X, U, t, n_in = _ragged_slab(list(X) if batched else [X])
    else:
        X = _f64(X)
        batched = X.ndim == 3
    if None in (MU, DU, TU, Isp) or n_new is None:
        raise ValueError("direct_resample: MU, DU, TU, Isp and n_new are required")
    X = _f64(X)
    U = _f64(U)
    ns, n, B, _ = _batch_dims(X)
    if ns not in (6, 7):
        raise ValueError("direct_resample: X must have 6 or 7 rows; got shape %s" % (X.shape,))
    if U.shape != (3,) + X.shape[1:]:
        raise ValueError("direct_resample: U must be [3 x n_cap] or [3 x n_cap x n_batch], as X; got shape %s" % (U.shape,))
    tt, ntg = _tgrids(t, n, B)
    if ntg != B:
        tt = np.asfortranarray(np.repeat(tt[:, None], B, axis=1))
    if n_in is not None:
        n_in = np.ascontiguousarray(np.atleast_1d(n_in), dtype=np.int32)
        if n_in.shape != (B,):
            raise ValueError("direct_resample: n_in must have one entry per trajectory")
    if weights is not None:
        weights = _f64(weights)
        if weights.shape != (n - 1,) + X.shape[2:]:
            raise ValueError("direct_resample: weights must be [(n_cap-1)] or [(n_cap-1) x n_batch]")
    ctx = ctx or default_context()
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    n_new = int(n_new)
    m = max(n_new, 2)
    Xo = np.empty((ns, m, B), order="F")
    Uo = np.empty((3, m, B), order="F")
    to = np.empty((m, B), order="F")
    eb = np.empty((n - 1, B), order="F")
    ea = np.empty((m - 1, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("direct_resample_batch")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(tt), _ptr(n_in) if n_in is not None else None,
                                              int(nsteps), C.byref(prm), n_new, _ptr(weights) if weights is not None else None,
                                              float(w_floor), int(passes), _ptr(Xo), _ptr(Uo), _ptr(to), _ptr(eb), _ptr(ea),
                                              _ptr(status)))
    if not batched:
        return DirectResample(Xo[:, :, 0], Uo[:, :, 0], to[:, 0], eb[:, 0], ea[:, 0], int(status[0]))
    return DirectResample(Xo, Uo, to, eb, ea, status)


def direct_jacobian_blocks(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, ctx=None, out=None):
    """Compact direct Jacobian: (Jac_temp[nstate x nvar x (n-1)], ddefect_dtf[nstate x (n-1)], defect, errors);
    nvar = 2(nstate+3), variable order [x_i; x_{i+1}; u_i; u_{i+1}] (:125).  out = (Jac_temp, ddefect_dtf, defect, errors):
    Fortran-ordered float64 arrays with the trailing batch axis, written in place (e.g. from Context.pinned_empty)."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    nvar = 2 * (ns + 3)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    if out is not None:
        Jt, dtf, defect, errors = out
        shapes = ((ns, nvar, n - 1, B), (ns, n - 1, B), (ns, n - 1, B), (n - 1, B))
        _check_out(out, shapes, "%s" % (shapes,))
    else:
        Jt = np.zeros((ns, nvar, n - 1, B), order="F")
        dtf = np.zeros((ns, n - 1, B), order="F")
        defect = np.zeros((ns, n - 1, B), order="F")
        errors = np.zeros((n - 1, B), order="F")
    ctx.check(ctx.fn("direct_jacobian")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm),
                                          _ptr(Jt), _ptr(dtf), _ptr(defect), _ptr(errors)))
    if not batched:
        return Jt[:, :, :, 0], dtf[:, :, 0], defect[:, :, 0], errors[:, 0]
    return Jt, dtf, defect, errors


def direct_scatter(Jac_temp, ddefect_dtf=None):
    """Band scatter of the direct jacobianCalc (:146-162) and the tf column (:516):
    Jac_full [nstate(n-1) x n(nstate+3) (+1)]; state columns node-major, then control columns."""
    ns, nvar, S = Jac_temp.shape
    n = S + 1
    ncol = n * (ns + 3) + (1 if ddefect_dtf is not None else 0)
    J = np.zeros((ns * S, ncol))
    for i in range(S):
        r = slice(ns * i, ns * (i + 1))
        J[r, ns * i:ns * i + 2 * ns] = Jac_temp[:, :2 * ns, i]
        J[r, ns * n + 3 * i:ns * n + 3 * i + 6] = Jac_temp[:, 2 * ns:, i]
    if ddefect_dtf is not None:
        J[:, -1] = np.asarray(ddefect_dtf).reshape(-1, order="F")
    return J


def direct_endpoint_partials(Jac_temp, ddefect_dtf):
    """The three finite-difference blocks endpointPartials assembles (multiShoot_CRTBP_direct.jl:168-246), read off the
    analytic Jacobian blocks instead of re-propagating:
      ddefect_dt     [nstate(n-1)]  partial of all defects wrt tf               (:176-190)  = the tf column
      d_defect1_dV1  [nstate x 3]   partial of defect 1 wrt an impulse at node 1 (:193-214)  = d defect_1 / d v_1
      d_defectN_dV2  [nstate x 3]   partial of defect N wrt an impulse at node n (:216-222)  = d defect_N / d v_n
    (the reference's tau1/tau2 columns use variables that are never defined, :232,:235; they are not reproduced)."""
    ns = Jac_temp.shape[0]
    return (np.asarray(ddefect_dtf).reshape(-1, order="F").copy(), Jac_temp[:, 3:6, 0].copy(),
            Jac_temp[:, ns + 3:ns + 6, -1].copy())


def direct_jacobianCalc(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, ctx=None, with_tf=True):
    """jacobianCalc (+ tf partial) of multiShoot_CRTBP_direct: Jac_full [nstate(n-1) x n(nstate+3)+1]."""
    Jt, dtf, _, _ = direct_jacobian_blocks(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, ctx)
    return direct_scatter(Jt, dtf if with_tf else None)


def direct_targets(s0, sf, mass, dV1, dV2):
    """lto_direct_targets: interpolated end states s0, sf (6 each), initial mass, current impulses dV1, dV2 (3 each)."""
    t = LtoDirectTargets()
    t.s0[:] = [float(v) for v in np.asarray(s0, dtype=np.float64).reshape(6)]
    t.sf[:] = [float(v) for v in np.asarray(sf, dtype=np.float64).reshape(6)]
    t.mass = float(mass)
    t.dV1[:] = [float(v) for v in np.asarray(dV1, dtype=np.float64).reshape(3)]
    t.dV2[:] = [float(v) for v in np.asarray(dV2, dtype=np.float64).reshape(3)]
    return t


def _targets_array(targets):
    """One lto_direct_targets or a sequence of them (one per trajectory) -> (ctypes array, count)."""
    if isinstance(targets, LtoDirectTargets):
        targets = [targets]
    arr = (LtoDirectTargets * len(targets))(*targets)
    return arr, len(targets)


def _direct_qp_call(name, n_p, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, ctx, extra=lambda ntgt: ()):
    """The marshalling the lto_direct_qp_step* entries share: extra(ntgt) gives the ctypes arguments between the targets and their
    count, n_p the number of p values per trajectory (0: the entry returns none)."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    tg, ntgt = _targets_array(targets)
    args = extra(ntgt)
    dX = np.zeros((ns, n, B), order="F")
    dU = np.zeros((3, n, B), order="F")
    dV = np.zeros((6, B), order="F")
    p = np.zeros((n_p, B), order="F")
    cost = np.zeros(B)
    ctx.check(ctx.fn(name)(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm), C.cast(tg, C.c_void_p),
                           *args, ntgt, 1 if allowImpulsive else 0, _ptr(dX), _ptr(dU), _ptr(dV), *((_ptr(p),) if n_p else ()),
                           _ptr(cost)))
    out = (dX, dU, dV) + ((p,) if n_p else ())
    if not batched:
        return tuple(a[..., 0] for a in out) + (float(cost[0]),)
    return out + (cost,)


def _direct_solve_call(name, n_hist, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, maxIter, ctx, orbits=None,
                       extra=lambda ntgt, B: ()):
    """The marshalling the lto_direct_solve*_batch entries share: the orbit tables of free ends go in front of the targets and make
    the entry return tau, extra(ntgt, B) gives the ctypes arguments between the targets' count and allowImpulsive, and the history
    has n_hist rows."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    ob = None if orbits is None else _orbits(orbits)
    tg, ntgt = _targets_array(targets)
    args = extra(ntgt, B)
    mi = int(maxIter)
    Xo = np.zeros((ns, n, B), order="F")
    Uo = np.zeros((3, n, B), order="F")
    dV = np.zeros((6, B), order="F")
    to = np.zeros((n, B), order="F")
    defect = np.zeros((ns, n - 1, B), order="F")
    tau_o = np.zeros((2, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    iters = np.zeros(B, dtype=np.int32)
    hist = np.full((n_hist, max(mi, 1), B), np.nan, order="F")
    free = ob is not None
    ctx.check(ctx.fn(name)(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm),
                           *((C.byref(ob.struct),) if free else ()), C.cast(tg, C.c_void_p), ntgt, *args, 1 if allowImpulsive else 0, mi,
                           _ptr(Xo), _ptr(Uo), _ptr(dV), _ptr(to), _ptr(defect), *((_ptr(tau_o),) if free else ()), _ptr(status),
                           _ptr(iters), _ptr(hist)))
    hist = hist[:, :mi]
    out = (Xo, Uo, dV, to, defect) + ((tau_o,) if free else ())
    if not batched:
        return tuple(a[..., 0] for a in out) + (int(status[0]), int(iters[0]), hist[:, :, 0])
    return out + (status, iters, hist)


def _end_models_array(models, ntgt):
    if isinstance(models, LtoDirectEndModel):
        models = [models]
    if len(models) != ntgt:
        raise ValueError("need as many end models as targets")
    return (LtoDirectEndModel * ntgt)(*models)


def _betas(beta, ntgt):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1), (ntgt,)))


def _taus(tau, B):
    return np.asfortranarray(np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(2, -1), (2, B)))


def direct_qp_step(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive=False, ctx=None):
    """One Jacobian sweep and one QP step of the direct method (optimizeTraj, direct.jl:248-403, for flagEnd = false, beta = 0,
    tf fixed) on the device: returns (x_update[nstate x n], u_update[3 x n], dV_update[6] = (dV1_jump; dV2_jump), cost).
    A trailing batch axis on X_all / u_all solves several problems at once (targets: one, or one per trajectory); the outputs
    then carry it too.  A singular KKT system raises LtoError(LTO_ESINGULAR)."""
    return _direct_qp_call("direct_qp_step", 0, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, ctx)


def costate_scale(DU, TU):
    """c of a = c u: the controls of the direct method are in N, the acceleration of the 6-state right-hand side in DU/TU^2 for its
    literal mass of 1000 kg (c = TU^2 / DU / 1e3 / 1000, formed as the library forms it).  The indirect method's costates are
    c^2 times the direct transcription's."""
    return (float(TU) * float(TU)) / float(DU) / 1e3 / 1000.0


def direct_costates(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive=False, with_XC=None, ctx=None):
    """Costates of direct solutions from the multipliers of a frozen QP step at the given point (lto_direct_costates_batch: one
    Jacobian sweep, one QP step, one kernel).  Returns (Lambda [nstate x n], mult [nstate x (n-1)], XC [12 x n] =
    (X; c^2 Lambda) with c = costate_scale(DU, TU) -- or None, kkt_res, status); a trailing batch axis on X_all / u_all does several
    at once.  with_XC: default nstate == 6 (the 14-dim hand-over is not built: nstate 7 with XC raises LTO_EUNSUPPORTED).  status
    1: that trajectory's KKT system is singular and its outputs are NaN."""
    ctx = ctx or default_context()
    X = _f64(X_all)
    U = _f64(u_all)
    ns, n, B, batched = _batch_dims(X)
    t, ntg = _tgrids(t_TU, n, B)
    prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
    tg, ntgt = _targets_array(targets)
    want_xc = (ns == 6) if with_XC is None else bool(with_XC)
    Lam = np.zeros((ns, n, B), order="F")
    mult = np.zeros((ns, n - 1, B), order="F")
    XC = np.zeros((12, n, B), order="F") if want_xc else None
    res = np.zeros(B)
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("direct_costates_batch")(ctx.handle, ns, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, int(nsteps), C.byref(prm),
                                              C.cast(tg, C.c_void_p), ntgt, 1 if allowImpulsive else 0, _ptr(Lam), _ptr(mult),
                                              _ptr(XC) if want_xc else None, _ptr(res), _ptr(status)))
    if not batched:
        return Lam[..., 0], mult[..., 0], (XC[..., 0] if want_xc else None), float(res[0]), int(status[0])
    return Lam, mult, XC, res, status


def direct_solve(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive=False, maxIter=100, ctx=None):
    """The loop of multiShoot_CRTBP_direct (direct.jl:477-594) on the device, trajectories resident in HBM (lto_direct_solve_batch).
    Returns (X_all, u_all, dV[6] = (dV1; dV2), t_TU, defect, status, iterations, history[3 x maxIter] = (max|defect|, cost, alpha));
    status 0 converged, 1 maxIter, 2 NaN, 3 singular KKT system.  A trailing batch axis solves several problems in one loop."""
    return _direct_solve_call("direct_solve_batch", 3, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, maxIter,
                              ctx)


class DirectOrbits:
    """lto_direct_orbits over the two orbit tables of the free-end model (times [n], states [>= 6 x n]); keeps the arrays alive."""

    def __init__(self, X0_times, X0_states, Xf_times, Xf_states):
        self._keep = [np.ascontiguousarray(X0_times, dtype=np.float64).reshape(-1),
                      np.asfortranarray(np.asarray(X0_states, dtype=np.float64)[:6]),
                      np.ascontiguousarray(Xf_times, dtype=np.float64).reshape(-1),
                      np.asfortranarray(np.asarray(Xf_states, dtype=np.float64)[:6])]
        t0, X0, tf, Xf = self._keep
        if X0.shape != (6, t0.size) or Xf.shape != (6, tf.size):
            raise ValueError("orbit tables: states must be [6 x n] with n the number of times")
        self.struct = LtoDirectOrbits(int(t0.size), int(tf.size), _ptr(t0), _ptr(X0), _ptr(tf), _ptr(Xf))


def direct_end_model(g0, gf, c0_norm, cf_norm):
    """lto_direct_end_model: g0, gf (6 each) and the 2-norms of c0, cf."""
    m = LtoDirectEndModel()
    m.g0[:] = [float(v) for v in np.asarray(g0, dtype=np.float64).reshape(6)]
    m.gf[:] = [float(v) for v in np.asarray(gf, dtype=np.float64).reshape(6)]
    m.c0_norm, m.cf_norm = float(c0_norm), float(cf_norm)
    return m


def _orbits(orbits):
    return orbits if isinstance(orbits, DirectOrbits) else DirectOrbits(*orbits)


def direct_end_states(tau, orbits, ctx=None):
    """End targets and end model of the free-end step on the device (lto_direct_end_states).  tau [2] or [2 x B] = (tau1; tau2);
    orbits = DirectOrbits or (X0_times, X0_states, Xf_times, Xf_states).  Returns (s0, sf, g0, gf, c0_norm, cf_norm) with a
    trailing batch axis when tau has one."""
    ctx = ctx or default_context()
    ob = _orbits(orbits)
    tau = np.asarray(tau, dtype=np.float64)
    batched = tau.ndim == 2
    tau = np.asfortranarray(tau.reshape(2, -1))
    B = tau.shape[1]
    s = np.zeros((12, B), order="F")
    model = (LtoDirectEndModel * B)()
    ctx.check(ctx.fn("direct_end_states")(ctx.handle, C.byref(ob.struct), B, _ptr(tau), _ptr(s), C.cast(model, C.c_void_p)))
    g0 = np.array([list(m.g0) for m in model]).T
    gf = np.array([list(m.gf) for m in model]).T
    c0 = np.array([m.c0_norm for m in model])
    cf = np.array([m.cf_norm for m in model])
    if not batched:
        return s[:6, 0], s[6:, 0], g0[:, 0], gf[:, 0], float(c0[0]), float(cf[0])
    return s[:6], s[6:], g0, gf, c0, cf


StackGuess = collections.namedtuple("StackGuess", "X t tau1 tau2_0 tau2 gap status")


def stack_guess(tau1, tof1, tof2, n_nodes, orbits, MU=MU, integ=None, ctx=None):
    """Trajectory-stacking initial guesses on the device (lto_stack_guess_batch; the reference demo's block,
    CRTBP_Multishoot_direct_demo.jl:116-157): per start a ballistic coast of tof1 TU on the departure orbit from phase tau1, the
    closest point of the arrival orbit (find_tau), a coast of tof2 TU from there, both sampled at LinRange(0, tof1 + tof2, n_nodes),
    the last node snapped onto the arrival orbit.  tau1, tof1, tof2: scalars, or arrays broadcast to one batch of B starts;
    orbits = DirectOrbits or (X0_times, X0_states, Xf_times, Xf_states).  Returns StackGuess(X [6 x n x B], t [n x B], tau1 [B]
    (wrapped into [0, 1]), tau2_0 [B] (junction), tau2 [B] (end), gap [2 x B] (the distances find_tau minimised), status [B]: 0, or
    2 where a node is not finite) -- without the batch axis when all three are scalars."""
    ctx = ctx or default_context()
    integ = integ or integrator()
    ob = _orbits(orbits)
    args = [np.asarray(v, dtype=np.float64) for v in (tau1, tof1, tof2)]
    batched = any(v.ndim > 0 for v in args)
    t1, f1, f2 = (np.ascontiguousarray(v) for v in np.broadcast_arrays(*(v.reshape(-1) for v in args)))
    B, n = t1.size, int(n_nodes)
    X = np.zeros((6, max(n, 0), B), order="F")
    t = np.zeros((max(n, 0), B), order="F")
    tau = np.zeros((3, B), order="F")
    gap = np.zeros((2, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("stack_guess_batch")(ctx.handle, n, B, float(MU), C.byref(ob.struct), C.byref(integ), _ptr(t1), _ptr(f1), _ptr(f2),
                                          _ptr(X), _ptr(t), _ptr(tau), _ptr(gap), _ptr(status)))
    if not batched:
        return StackGuess(X[:, :, 0], t[:, 0], float(tau[0, 0]), float(tau[1, 0]), float(tau[2, 0]), gap[:, 0], int(status[0]))
    return StackGuess(X, t, tau[0].copy(), tau[1].copy(), tau[2].copy(), gap, status)


HALO_HOLD_Z0, HALO_HOLD_X0, HALO_PLANAR = 0, 1, 2
_HALO_MODES = {"z0": HALO_HOLD_Z0, "hold_z0": HALO_HOLD_Z0, "x0": HALO_HOLD_X0, "hold_x0": HALO_HOLD_X0, "planar": HALO_PLANAR}
HaloCorrect = collections.namedtuple("HaloCorrect", "state period resid iterations history status")
HaloTable = collections.namedtuple("HaloTable", "times X M closure jacobi nu status")


def _halo_mode(mode):
    if isinstance(mode, str):
        if mode not in _HALO_MODES:
            raise ValueError("mode must be 'z0' (hold z0), 'x0' (hold x0) or 'planar'")
        return _HALO_MODES[mode]
    if mode not in (HALO_HOLD_Z0, HALO_HOLD_X0, HALO_PLANAR):
        raise ValueError("mode must be HALO_HOLD_Z0, HALO_HOLD_X0 or HALO_PLANAR")
    return int(mode)


def halo_correct(seeds, mode, tol=1e-12, max_iter=15, t_max=10.0, MU=MU, sing_tol=1e-12, integ=None, ctx=None):
    """The differential corrector of periodic orbits with the xz-plane symmetry on the device (lto_halo_correct_batch, DESIGN
    4.25).  seeds [6] or [6 x B]: (x0, ., z0, ., vy0, .), the flight starts at (x0, 0, z0, 0, vy0, 0); mode 'z0' (hold z0: x0 and
    vy0 move), 'x0' (hold x0: z0 and vy0 move) or 'planar' (z0 = 0, vy0 moves) -- or the HALO_* constants.  The first return to
    y = 0 is searched up to t_max (TU); with RK4 integ.steps steps span t_max.  Returns HaloCorrect(state [6 x B], period [B],
    resid [B], iterations [B], history [(max_iter + 1) x B] (NaN past the last flight), status [B]: 0 converged, 1 max_iter
    reached, 2 unusable seed or flight, 3 singular step) -- without the batch axis for a single seed."""
    mode = _halo_mode(mode)                       # the shapes and the mode are checked before any library call
    S = np.asarray(seeds, dtype=np.float64)
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("seeds must be [6] or [6 x B]")
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be >= 0")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    ctx = ctx or default_context()
    integ = integ or integrator()
    state = np.zeros((6, B), order="F")
    period = np.zeros(B)
    resid = np.zeros(B)
    hist = np.zeros((max_iter + 1, B), order="F")
    its = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("halo_correct_batch")(ctx.handle, B, float(MU), mode, _ptr(S), float(tol), max_iter, float(t_max), float(sing_tol),
                                           C.byref(integ), _ptr(state), _ptr(period), _ptr(resid), _ptr(its), _ptr(hist), _ptr(status)))
    if not batched:
        return HaloCorrect(state[:, 0], float(period[0]), float(resid[0]), int(its[0]), hist[:, 0], int(status[0]))
    return HaloCorrect(state, period, resid, its, hist, status)


HALO_TARGET_JACOBI, HALO_TARGET_PERIOD = 0, 1
_HALO_TARGETS = {"jacobi": HALO_TARGET_JACOBI, "period": HALO_TARGET_PERIOD}
HaloTarget = collections.namedtuple("HaloTarget", "state period jacobi resid iterations history status")


def halo_target(seeds, targets, what="jacobi", planar=False, tol=1e-12, max_iter=15, t_max=10.0, MU=MU, sing_tol=1e-12, integ=None,
                ctx=None):
    """Periodic orbits at a given Jacobi constant (what = 'jacobi') or period ('period') on the device (lto_halo_target_batch,
    DESIGN 4.27): the corrector of halo_correct with (x0, z0, vy0) -- planar: (x0, vy0), z0 = 0 -- as unknowns and q - q* as a third
    residual.  seeds [6] or [6 x B]; targets a scalar (every orbit's one target), [K] (the K members of a march, the same for every
    orbit) or [K x B]: orbit b's members are corrected one after another in the one launch, each from the secant through the last
    two.  Returns HaloTarget(state [6 x K x B], period, jacobi, resid, iterations [K x B], history [(max_iter + 1) x K x B] (NaN past
    the last flight), status [K x B]: 0 converged, 1 max_iter reached, 2 unusable, 3 singular step) -- without the batch axis for
    a single seed and without the target axis for a scalar target."""
    if isinstance(what, str):                     # shapes, enumerations and finiteness are checked before any library call
        if what not in _HALO_TARGETS:
            raise ValueError("what must be 'jacobi' or 'period'")
        what = _HALO_TARGETS[what]
    elif what not in (HALO_TARGET_JACOBI, HALO_TARGET_PERIOD):
        raise ValueError("what must be HALO_TARGET_JACOBI or HALO_TARGET_PERIOD")
    S = np.asarray(seeds, dtype=np.float64)
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("seeds must be [6] or [6 x B]")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    Q = np.asarray(targets, dtype=np.float64)
    marched = Q.ndim >= 1
    if Q.ndim > 2 or Q.size == 0 or (Q.ndim == 2 and (not batched or Q.shape[1] != B)):
        raise ValueError("targets must be a scalar, [K] or, with seeds [6 x B], [K x B]")
    K = Q.shape[0] if marched else 1
    Q = np.asfortranarray(np.broadcast_to(Q.reshape(K, -1), (K, B)))
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be >= 0")
    tol, t_max, sing_tol = float(tol), float(t_max), float(sing_tol)
    if not (tol > 0.0) or not (np.isfinite(t_max) and t_max > 0.0) or not (0.0 <= sing_tol < 1.0):
        raise ValueError("need tol > 0, t_max finite and > 0, sing_tol in [0, 1)")
    ctx = ctx or default_context()
    integ = integ or integrator()
    state = np.zeros((6, K, B), order="F")
    period, jac, resid = np.zeros((K, B), order="F"), np.zeros((K, B), order="F"), np.zeros((K, B), order="F")
    hist = np.zeros((max_iter + 1, K, B), order="F")
    its = np.zeros((K, B), dtype=np.int32, order="F")
    status = np.zeros((K, B), dtype=np.int32, order="F")
    ctx.check(ctx.fn("halo_target_batch")(ctx.handle, K, B, float(MU), int(bool(planar)), int(what), _ptr(S), _ptr(Q), tol, max_iter, t_max,
                                          sing_tol, C.byref(integ), _ptr(state), _ptr(period), _ptr(jac), _ptr(resid), _ptr(its),
                                          _ptr(hist), _ptr(status)))
    out = [state, period, jac, resid, its, hist, status]
    if not batched:
        out = [o[..., 0] for o in out]
    if not marched:
        out = [out[0][:, 0]] + [o[0] for o in out[1:5]] + [out[5][:, 0], out[6][0]]
    if not batched and not marched:
        out = [out[0], float(out[1]), float(out[2]), float(out[3]), int(out[4]), out[5], int(out[6])]
    return HaloTarget(*out)


HaloArclength = collections.namedtuple("HaloArclength",
                                       "state tangent det ds halvings period jacobi resid iterations history status")


def halo_arclength(seeds, n_members, ds, direction, planar=False, dir_is_tangent=False, ds_min=None, ds_max=None, grow=1.0, fast_iter=3,
                   cos_min=0.0, tol=1e-12, max_iter=15, t_max=10.0, MU=MU, sing_tol=1e-12, integ=None, ctx=None):
    """A family of periodic orbits by pseudo-arclength continuation on the device (lto_halo_arclength_batch): the
    unknowns (x0, z0, vy0) -- planar: (x0, vy0), z0 = 0 -- move along the family's tangent, so that the march passes the folds of
    every coordinate, of the Jacobi constant and of the period.  seeds [6] or [6 x B]; ds a scalar or [B], the first step;
    direction [3] or [3 x B] in (x0, z0, vy0).  dir_is_tangent = False: member 0 is the seed corrected onto the family, and the
    march leaves it towards the side of `direction`; True: the seed is a point of the family, `direction` its tangent (used as
    given) and member 0 the step from it by ds -- from a branch point with direction (0, +-1, 0) onto the family born there.  A
    failed attempt (not converged in max_iter steps, or the tangent turned beyond cos_min) is tried again with ds / 2 down to
    ds_min (default: the smallest ds / 1024); after a member of <= fast_iter steps ds grows by `grow` up to ds_max (default: the
    largest ds).  Returns HaloArclength(state [6 x K x B], tangent [3 x K x B], det (its sign changes where another family branches
    off), ds (the accepted steps), halvings, period, jacobi, resid, iterations [K x B], history [(max_iter + 1) x K x B], status
    [K x B]: 0 converged, 1 max_iter reached, 2 unusable, 3 singular step or no tangent, 4 the tangent turned beyond cos_min; any
    status but 0 ends the orbit's march, the rest is NaN with status 2) -- without the batch axis for a single seed."""
    S = np.asarray(seeds, dtype=np.float64)       # shapes and values are checked before any library call
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("seeds must be [6] or [6 x B]")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    K = int(n_members)
    if K < 1:
        raise ValueError("n_members must be >= 1")
    D = np.asarray(direction, dtype=np.float64)
    if D.ndim not in (1, 2) or D.shape[0] != 3 or (D.ndim == 2 and (not batched or D.shape[1] != B)):
        raise ValueError("direction must be [3] or, with seeds [6 x B], [3 x B]")
    D = np.asfortranarray(np.broadcast_to(D.reshape(3, -1), (3, B)))
    s0 = np.asarray(ds, dtype=np.float64)
    if s0.ndim > 1 or (s0.ndim == 1 and (not batched or s0.size != B)):
        raise ValueError("ds must be a scalar or, with seeds [6 x B], [B]")
    s0 = np.ascontiguousarray(np.broadcast_to(s0.reshape(-1), (B,)))
    if not np.all(np.isfinite(s0)) or not np.all(s0 > 0.0):
        raise ValueError("ds must be finite and > 0")
    ds_min = float(s0.min() / 1024.0 if ds_min is None else ds_min)
    ds_max = float(s0.max() if ds_max is None else ds_max)
    grow, cos_min, fast_iter, max_iter = float(grow), float(cos_min), int(fast_iter), int(max_iter)
    if not (ds_min > 0.0) or not (ds_min <= ds_max) or not np.isfinite(ds_max):
        raise ValueError("need 0 < ds_min <= ds_max, both finite")
    if not (grow >= 1.0) or not np.isfinite(grow) or fast_iter < 0 or not (0.0 <= cos_min < 1.0):
        raise ValueError("need grow finite and >= 1, fast_iter >= 0, cos_min in [0, 1)")
    if max_iter < 0:
        raise ValueError("max_iter must be >= 0")
    tol, t_max, sing_tol = float(tol), float(t_max), float(sing_tol)
    if not (tol > 0.0) or not (np.isfinite(t_max) and t_max > 0.0) or not (0.0 <= sing_tol < 1.0):
        raise ValueError("need tol > 0, t_max finite and > 0, sing_tol in [0, 1)")
    ctx = ctx or default_context()
    integ = integ or integrator()
    state, tangent = np.zeros((6, K, B), order="F"), np.zeros((3, K, B), order="F")
    det, dso, period, jac, resid = (np.zeros((K, B), order="F") for _ in range(5))
    hist = np.zeros((max_iter + 1, K, B), order="F")
    halv, its, status = (np.zeros((K, B), dtype=np.int32, order="F") for _ in range(3))
    ctx.check(ctx.fn("halo_arclength_batch")(ctx.handle, K, B, float(MU), int(bool(planar)), int(bool(dir_is_tangent)), _ptr(S), _ptr(D),
                                             _ptr(s0), ds_min, ds_max, grow, fast_iter, cos_min, tol, max_iter, t_max, sing_tol,
                                             C.byref(integ), _ptr(state), _ptr(tangent), _ptr(det), _ptr(dso), _ptr(halv), _ptr(period),
                                             _ptr(jac), _ptr(resid), _ptr(its), _ptr(hist), _ptr(status)))
    out = [state, tangent, det, dso, halv, period, jac, resid, its, hist, status]
    if not batched:
        out = [o[..., 0] for o in out]
    return HaloArclength(*out)


def halo_table(state0, period, n_samples, MU=MU, integ=None, ctx=None):
    """One revolution of periodic orbits on the device, sampled at n_samples equal times with the state-transition matrix carried
    through (lto_halo_table_batch).  state0 [6] or [6 x B], period scalar or [B].  Returns HaloTable(times [n] = i /
    (n - 1), X [6 x n x B], M [6 x 6 x B] = Phi(P), closure [B], jacobi [2 x B] = (C, largest drift over the samples), nu [2 x B]
    (stability indices), status [B]: 0, or 2 without a finite result) -- without the batch axis for a single orbit.  (times, X) is
    what DirectOrbits takes."""
    S = np.asarray(state0, dtype=np.float64)
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("state0 must be [6] or [6 x B]")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    P = np.ascontiguousarray(np.broadcast_to(np.asarray(period, dtype=np.float64).reshape(-1), (B,)))
    n = int(n_samples)
    if n < 2:
        raise ValueError("n_samples must be >= 2")
    ctx = ctx or default_context()
    integ = integ or integrator()
    X = np.zeros((6, n, B), order="F")
    times = np.zeros(n)
    M = np.zeros((6, 6, B), order="F")
    closure = np.zeros(B)
    jac = np.zeros((2, B), order="F")
    nu = np.zeros((2, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("halo_table_batch")(ctx.handle, n, B, float(MU), _ptr(S), _ptr(P), C.byref(integ), _ptr(X), _ptr(times), _ptr(M),
                                         _ptr(closure), _ptr(jac), _ptr(nu), _ptr(status)))
    if not batched:
        return HaloTable(times, X[:, :, 0], M[:, :, 0], float(closure[0]), jac[:, 0], nu[:, 0], int(status[0]))
    return HaloTable(times, X, M, closure, jac, nu, status)


ManifoldSeeds = collections.namedtuple("ManifoldSeeds", "lam X V starts tau status")
SectionFlight = collections.namedtuple("SectionFlight", "x_end t_end count dC X status")
StateMatch = collections.namedtuple("StateMatch", "index dist dr dv")
_SECTION_AXES = {"x": 0, "y": 1, "z": 2, "vx": 3, "vy": 4, "vz": 5}


def _flight_integrator(integ):
    integ = integ or integrator()
    if integ.method not in (RK4, DOP853_ADAPTIVE):
        raise ValueError("the flight is built for RK4 and DOP853_ADAPTIVE")
    if integ.method == RK4 and integ.steps < 1:
        raise ValueError("RK4 needs steps >= 1")
    return integ


def manifold_seeds(state0, period, M, tau, eps=1e-6, MU=MU, integ=None, ctx=None):
    """The hyperbolic eigen-directions of periodic orbits at the phases tau and the perturbed manifold starts
    (lto_halo_manifold_seeds_batch).  state0 [6] or [6 x B], period scalar or [B], M [6 x 6] or [6 x 6 x B] as
    halo_table returns it, tau [P] (any finite values; they are wrapped into [0, 1)), eps the offset in the 6-norm of (DU, DU / TU).
    Returns ManifoldSeeds(lam [2 x B] = (lambda_u, lambda_s), X [6 x 2 x P x B] the orbit point as the (unstable, stable) flight
    reached it, V [6 x 2 x P x B] the unit vectors there, starts [6 x 4 x P x B] = X +- eps V in the order (u+, u-, s+, s-), tau [P]
    as wrapped, status [B]: 0, 1 no usable hyperbolic pair, 2 a flight without a finite result) -- without the batch axis for a
    single orbit."""
    S = np.asarray(state0, dtype=np.float64)
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("state0 must be [6] or [6 x B]")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    Mm = np.asarray(M, dtype=np.float64)
    if Mm.shape != ((6, 6, B) if batched else (6, 6)):
        raise ValueError("M must be [6 x 6] for one orbit, [6 x 6 x B] for a batch")
    Mm = np.asfortranarray(Mm.reshape(6, 6, B))
    P = np.asarray(period, dtype=np.float64).reshape(-1)
    if P.size not in (1, B):
        raise ValueError("period must be a scalar or [B]")
    P = np.ascontiguousarray(np.broadcast_to(P, (B,)))
    tau = np.ascontiguousarray(np.asarray(tau, dtype=np.float64).reshape(-1))
    if tau.size < 1 or not np.all(np.isfinite(tau)):
        raise ValueError("tau must hold at least one phase, all finite")
    eps = float(eps)
    if not (np.isfinite(eps) and eps > 0.0):
        raise ValueError("eps must be finite and > 0")
    integ = _flight_integrator(integ)
    ctx = ctx or default_context()
    n = tau.size
    lam = np.zeros((2, B), order="F")
    X = np.zeros((6, 2, n, B), order="F")
    V = np.zeros((6, 2, n, B), order="F")
    starts = np.zeros((6, 4, n, B), order="F")
    status = np.zeros(B, dtype=np.int32)
    ctx.check(ctx.fn("halo_manifold_seeds_batch")(ctx.handle, n, B, float(MU), _ptr(S), _ptr(P), _ptr(Mm), _ptr(tau), eps, C.byref(integ),
                                                  _ptr(lam), _ptr(X), _ptr(V), _ptr(starts), _ptr(status)))
    wrapped = tau - np.floor(tau)
    wrapped[wrapped >= 1.0] = 0.0
    if not batched:
        return ManifoldSeeds(lam[:, 0], X[..., 0], V[..., 0], starts[..., 0], wrapped, int(status[0]))
    return ManifoldSeeds(lam, X, V, starts, wrapped, status)


def section_flight(y0, t_max, section=("y", 0.0), sec_dir=0, n_cross=1, r_min=(0.0, 0.0), n_samples=0, MU=MU, integ=None, ctx=None):
    """Ballistic CRTBP arcs flown to a Poincare section (lto_section_flight_batch), one lane per arc.  y0 [6] or [6 x N];
    t_max scalar or [N], SIGNED (negative: backward in time), finite and non-zero; section = (axis, value) with axis 0..5 or one of
    'x', 'y', 'z', 'vx', 'vy', 'vz'; sec_dir +1 / -1 counts sign changes of g = y[axis] - value from - to + / + to - in the order
    the flight visits the points (for a backward arc the opposite of the physical sense), 0 both; the n_cross-th counted crossing ends
    the arc (n_cross = 0: no section, fly to t_max); r_min = distances from the two primaries that end an arc with status 3 (0: off);
    n_samples = 0, or >= 2 for samples at k t_max / (n_samples - 1).  Returns SectionFlight(x_end [6 x N], t_end [N] signed, count
    [N], dC [N] the Jacobi constant's drift, X [6 x n_samples x N] or None, status [N]: 0 ended as asked, 1 t_max reached first,
    2 no finite result, 3 inside r_min) -- without the batch axis for a single arc."""
    Y = np.asarray(y0, dtype=np.float64)
    if Y.ndim not in (1, 2) or Y.shape[0] != 6 or Y.size == 0:
        raise ValueError("y0 must be [6] or [6 x N]")
    batched = Y.ndim == 2
    Y = np.asfortranarray(Y.reshape(6, -1))
    N = Y.shape[1]
    T = np.asarray(t_max, dtype=np.float64).reshape(-1)
    if T.size not in (1, N):
        raise ValueError("t_max must be a scalar or [N]")
    T = np.ascontiguousarray(np.broadcast_to(T, (N,)))
    if not np.all(np.isfinite(T)) or np.any(T == 0.0):
        raise ValueError("every t_max must be finite and non-zero")
    try:
        axis, value = section
    except (TypeError, ValueError):
        raise ValueError("section must be (axis, value)")
    if isinstance(axis, str):
        if axis not in _SECTION_AXES:
            raise ValueError("section axis must be 0..5 or one of 'x', 'y', 'z', 'vx', 'vy', 'vz'")
        axis = _SECTION_AXES[axis]
    if axis not in (0, 1, 2, 3, 4, 5):
        raise ValueError("section axis must be 0..5 or one of 'x', 'y', 'z', 'vx', 'vy', 'vz'")
    value = float(value)
    if not np.isfinite(value):
        raise ValueError("the section's value must be finite")
    if sec_dir not in (-1, 0, 1):
        raise ValueError("sec_dir must be -1, 0 or +1")
    n_cross, n_samples = int(n_cross), int(n_samples)
    if n_cross < 0:
        raise ValueError("n_cross must be >= 0")
    if n_samples < 0 or n_samples == 1:
        raise ValueError("n_samples must be 0 or >= 2")
    R = np.ascontiguousarray(np.asarray(r_min, dtype=np.float64).reshape(-1))
    if R.size != 2 or not np.all(np.isfinite(R)) or np.any(R < 0.0):
        raise ValueError("r_min must hold two finite distances >= 0")
    integ = _flight_integrator(integ)
    ctx = ctx or default_context()
    x_end = np.zeros((6, N), order="F")
    t_end = np.zeros(N)
    dC = np.zeros(N)
    count = np.zeros(N, dtype=np.int32)
    status = np.zeros(N, dtype=np.int32)
    X = np.zeros((6, n_samples, N), order="F") if n_samples else None
    ctx.check(ctx.fn("section_flight_batch")(ctx.handle, N, float(MU), _ptr(Y), _ptr(T), int(axis), value, int(sec_dir), n_cross, _ptr(R),
                                             n_samples, C.byref(integ), _ptr(x_end), _ptr(t_end), _ptr(count), _ptr(dC), _ptr(X),
                                             _ptr(status)))
    if not batched:
        return SectionFlight(x_end[:, 0], float(t_end[0]), int(count[0]), float(dC[0]), None if X is None else X[:, :, 0], int(status[0]))
    return SectionFlight(x_end, t_end, count, dC, X, status)


def state_match(A, Bs, w=1.0, ctx=None):
    """For each state of A [6] or [6 x nA] the nearest of Bs [6 x nB] in d = sqrt(|dr|^2 + (w |dv|)^2) (lto_state_match_batch, DESIGN
    4.26): the lowest index on ties, a NaN distance never wins, index -1 and NaN where every distance is NaN.  Returns
    StateMatch(index [nA], dist [nA], dr [nA], dv [nA]) -- scalars for a single state of A."""
    Aa = np.asarray(A, dtype=np.float64)
    if Aa.ndim not in (1, 2) or Aa.shape[0] != 6 or Aa.size == 0:
        raise ValueError("A must be [6] or [6 x nA]")
    Bb = np.asarray(Bs, dtype=np.float64)
    if Bb.ndim != 2 or Bb.shape[0] != 6 or Bb.size == 0:
        raise ValueError("Bs must be [6 x nB]")
    w = float(w)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("w must be finite and >= 0")
    batched = Aa.ndim == 2
    Aa = np.asfortranarray(Aa.reshape(6, -1))
    Bb = np.asfortranarray(Bb)
    nA, nB = Aa.shape[1], Bb.shape[1]
    ctx = ctx or default_context()
    index = np.zeros(nA, dtype=np.int32)
    dist = np.zeros(nA)
    dr = np.zeros(nA)
    dv = np.zeros(nA)
    ctx.check(ctx.fn("state_match_batch")(ctx.handle, nA, nB, _ptr(Aa), _ptr(Bb), w, _ptr(index), _ptr(dist), _ptr(dr), _ptr(dv)))
    if not batched:
        return StateMatch(int(index[0]), float(dist[0]), float(dr[0]), float(dv[0]))
    return StateMatch(index, dist, dr, dv)


StationkeepGains = collections.namedtuple("StationkeepGains", "W G alpha status")
StationkeepFlight = collections.namedtuple(
    "StationkeepFlight", "x_final dv_total n_burn dev dv_hist dev_final accepted rejected status lost_at")


def stationkeep_gains(V, sing_tol=1e-8, ctx=None):
    """The Floquet-mode station-keeping gains from the hyperbolic directions of manifold_seeds (lto_stationkeep_gains_batch, DESIGN
    4.29).  V [6 x 2 x P] or [6 x 2 x P x B], ManifoldSeeds.V as it is (index 0 the unstable unit vector, 1 the stable one).
    Returns StationkeepGains(W [6 x P x B] = S v_s scaled so that W . v_u = 1, the left eigenvector of the monodromy matrix for
    lambda_u; G [3 x 6 x P x B] = -w_v W^T / |w_v|^2, w_v = W[3:6]: dv = G dx is the smallest velocity change that zeroes the
    unstable component of dx; alpha [P x B] = |w_v| / |W|; status [P x B]: 0, 2 a non-finite input, 3 alpha <= sing_tol or
    |S v_s . v_u| <= sing_tol |S v_s| |v_u|; NaN outputs where status != 0) -- without the batch axis for [6 x 2 x P]."""
    Vv = np.asarray(V, dtype=np.float64)
    if Vv.ndim not in (3, 4) or Vv.shape[:2] != (6, 2) or Vv.size == 0:
        raise ValueError("V must be [6 x 2 x P] or [6 x 2 x P x B]")
    sing_tol = float(sing_tol)
    if not (0.0 <= sing_tol < 1.0):
        raise ValueError("sing_tol must lie in [0, 1)")
    batched = Vv.ndim == 4
    P = Vv.shape[2]
    Vv = np.asfortranarray(Vv.reshape(6, 2, P, -1, order="F"))
    B = Vv.shape[3]
    ctx = ctx or default_context()
    W = np.zeros((6, P, B), order="F")
    G = np.zeros((3, 6, P, B), order="F")
    alpha = np.zeros((P, B), order="F")
    status = np.zeros((P, B), dtype=np.int32, order="F")
    ctx.check(ctx.fn("stationkeep_gains_batch")(ctx.handle, P, B, _ptr(Vv), sing_tol, _ptr(W), _ptr(G), _ptr(alpha), _ptr(status)))
    if not batched:
        return StationkeepGains(W[..., 0], G[..., 0], alpha[:, 0], status[:, 0])
    return StationkeepGains(W, G, alpha, status)


def stationkeep_flight(X_ref, dt, G, x0, n_rev, nav=None, exe=None, dv_min=0.0, dv_max=0.0, r_lost=0.0, MU=MU, integ=None, ctx=None,
                       history=True):
    """Runs flown under an impulsive linear feedback about periodic orbits (lto_stationkeep_flight_batch), one lane per
    run.  X_ref [6 x n_man], dt [n_man], G [3 x 6 x n_man] (one orbit for every run) or [6 x n_man x B], [n_man x B], [3 x 6 x n_man x
    B] (one per run): the reference point, the gain and the ballistic span after burn j, every dt finite and > 0.  x0 [6] or [6 x
    B]: the state at the first burn epoch.  nav [6 x n_upd (x B)] and exe [4 x n_upd (x B)] or None, n_upd = n_rev n_man: the
    navigation error added to the measured deviation, and (scale error, bias [3]) of the executed burn.  At update u = r n_man + j:
    d = x - X_ref_j; lost if r_lost > 0 and |d_r| > r_lost; c = G_j (d + nav_u); no burn if |c| < dv_min; |c| clipped to dv_max
    (0: no limit); v += (1 + exe_0) c + exe_1:4; then the span dt_j.  Returns StationkeepFlight(x_final [6 x B], dv_total [B],
    n_burn [B], dev [2 x n_upd x B] = (|d_r|, |d_v|) at every update, dv_hist [n_upd x B] the applied |dv| (0: skipped), dev_final
    [2 x B] against X_ref_0 (a lost run: the deviation that lost it), accepted, rejected, status [B]: 0, 1 lost, 2 no finite
    result; lost_at [B] the update of the loss or -1) -- without the batch axis for a single start.  history=False leaves dev and
    dv_hist out (None): 24 n_upd bytes per run that a large Monte Carlo need not bring back."""
    X = np.asarray(x0, dtype=np.float64)
    if X.ndim not in (1, 2) or X.shape[0] != 6 or X.size == 0:
        raise ValueError("x0 must be [6] or [6 x B]")
    batched = X.ndim == 2
    X = np.asfortranarray(X.reshape(6, -1))
    B = X.shape[1]
    Xr = np.asarray(X_ref, dtype=np.float64)
    if Xr.ndim not in (2, 3) or Xr.shape[0] != 6 or Xr.size == 0:
        raise ValueError("X_ref must be [6 x n_man] or [6 x n_man x n_orb]")
    n_man = Xr.shape[1]
    Xr = np.asfortranarray(Xr.reshape(6, n_man, -1, order="F"))
    n_orb = Xr.shape[2]
    if n_orb != 1 and n_orb != B:
        raise ValueError("X_ref must hold one orbit or one per run")
    T = np.asarray(dt, dtype=np.float64)
    if T.size != n_man * n_orb or T.shape[0] != n_man:
        raise ValueError("dt must be [n_man] or [n_man x n_orb]")
    T = np.asfortranarray(T.reshape(n_man, n_orb, order="F"))
    if not np.all(np.isfinite(T)) or np.any(T <= 0.0):
        raise ValueError("every dt must be finite and > 0")
    Gg = np.asarray(G, dtype=np.float64)
    if Gg.size != 18 * n_man * n_orb or Gg.shape[:3] != (3, 6, n_man):
        raise ValueError("G must be [3 x 6 x n_man] or [3 x 6 x n_man x n_orb]")
    Gg = np.asfortranarray(Gg.reshape(3, 6, n_man, n_orb, order="F"))
    n_rev = int(n_rev)
    if n_rev < 1:
        raise ValueError("n_rev must be >= 1")
    n_upd = n_rev * n_man
    errs = []
    for name, arr, rows in (("nav", nav, 6), ("exe", exe, 4)):
        if arr is None:
            errs.append(None)
            continue
        E = np.asarray(arr, dtype=np.float64)
        if E.ndim not in (2, 3) or E.shape[0] != rows or E.shape[1] != n_upd or E.size not in (rows * n_upd, rows * n_upd * B):
            raise ValueError("%s must be [%d x n_upd] or [%d x n_upd x B] with n_upd = %d" % (name, rows, rows, n_upd))
        E = E.reshape(rows, n_upd, -1, order="F")
        errs.append(np.asfortranarray(np.broadcast_to(E, (rows, n_upd, B))))
    dv_min, dv_max, r_lost = float(dv_min), float(dv_max), float(r_lost)
    for name, v in (("dv_min", dv_min), ("dv_max", dv_max), ("r_lost", r_lost)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError("%s must be finite and >= 0" % name)
    integ = _flight_integrator(integ)
    ctx = ctx or default_context()
    x_final = np.zeros((6, B), order="F")
    dv_total = np.zeros(B)
    dev = np.zeros((2, n_upd, B), order="F") if history else None
    dv_hist = np.zeros((n_upd, B), order="F") if history else None
    dev_final = np.zeros((2, B), order="F")
    n_burn, acc, rej, status, lost_at = (np.zeros(B, dtype=np.int32) for _ in range(5))
    ctx.check(ctx.fn("stationkeep_flight_batch")(ctx.handle, n_man, n_rev, B, float(MU), _ptr(Xr), _ptr(T), _ptr(Gg), n_orb, _ptr(X),
                                                 _ptr(errs[0]), _ptr(errs[1]), dv_min, dv_max, r_lost, C.byref(integ), _ptr(x_final),
                                                 _ptr(dv_total), _ptr(n_burn), _ptr(dev), _ptr(dv_hist), _ptr(dev_final), _ptr(acc),
                                                 _ptr(rej), _ptr(status), _ptr(lost_at)))
    if not batched:
        return StationkeepFlight(x_final[:, 0], float(dv_total[0]), int(n_burn[0]), dev[:, :, 0] if history else None,
                                 dv_hist[:, 0] if history else None, dev_final[:, 0],
                                 int(acc[0]), int(rej[0]), int(status[0]), int(lost_at[0]))
    return StationkeepFlight(x_final, dv_total, n_burn, dev, dv_hist, dev_final, acc, rej, status, lost_at)


HaloStm = collections.namedtuple("HaloStm", "X Phi X_tgt tau horizons accepted rejected status")
StationkeepTargetGains = collections.namedtuple("StationkeepTargetGains", "G pivot status")


def _horizons(horizons):
    h = np.ascontiguousarray(np.asarray(horizons, dtype=np.float64).reshape(-1))
    if h.size < 1 or not np.all(np.isfinite(h)) or h[0] <= 0.0 or np.any(np.diff(h) <= 0.0):
        raise ValueError("horizons must hold at least one target, all finite, > 0 and strictly increasing")
    return h


def halo_stm(state0, period, tau, horizons, MU=MU, integ=None, ctx=None):
    """The state-transition matrices between phases of periodic orbits (lto_halo_stm_batch).  state0 [6] or [6 x B],
    period scalar or [B], tau [P] the phases (any finite values; they are wrapped into [0, 1)), horizons [K] in periods, finite, > 0
    and strictly increasing.  Returns HaloStm(X [6 x P x B] the orbit point at each phase, Phi [6 x 6 x K x P x B] = Phi(t_j + h_k
    period, t_j) with t_j = tau_j period, X_tgt [6 x K x P x B] the orbit point at each target, tau [P] as wrapped, horizons [K],
    accepted and rejected [P x B] the steps of the coast and the spans, status [P x B]: 0, or 2 without a finite result, NaN in that
    record) -- without the batch axis for a single orbit."""
    S = np.asarray(state0, dtype=np.float64)
    if S.ndim not in (1, 2) or S.shape[0] != 6 or S.size == 0:
        raise ValueError("state0 must be [6] or [6 x B]")
    batched = S.ndim == 2
    S = np.asfortranarray(S.reshape(6, -1))
    B = S.shape[1]
    P = np.asarray(period, dtype=np.float64).reshape(-1)
    if P.size not in (1, B):
        raise ValueError("period must be a scalar or [B]")
    P = np.ascontiguousarray(np.broadcast_to(P, (B,)))
    tau = np.ascontiguousarray(np.asarray(tau, dtype=np.float64).reshape(-1))
    if tau.size < 1 or not np.all(np.isfinite(tau)):
        raise ValueError("tau must hold at least one phase, all finite")
    h = _horizons(horizons)
    if not (0.0 < float(MU) < 1.0):
        raise ValueError("MU must lie in (0, 1)")
    n, K = tau.size, h.size
    if 36 * K * n * B > 0x7fffffff:
        raise ValueError("36 n_tgt n_phase n_batch must not exceed 2^31 - 1")
    integ = _flight_integrator(integ)
    ctx = ctx or default_context()
    X = np.zeros((6, n, B), order="F")
    Phi = np.zeros((6, 6, K, n, B), order="F")
    Xt = np.zeros((6, K, n, B), order="F")
    acc, rej, status = (np.zeros((n, B), dtype=np.int32, order="F") for _ in range(3))
    ctx.check(ctx.fn("halo_stm_batch")(ctx.handle, n, K, B, float(MU), _ptr(S), _ptr(P), _ptr(tau), _ptr(h), C.byref(integ), _ptr(X),
                                       _ptr(Phi), _ptr(Xt), _ptr(acc), _ptr(rej), _ptr(status)))
    wrapped = tau - np.floor(tau)
    wrapped[wrapped >= 1.0] = 0.0
    if not batched:
        return HaloStm(X[..., 0], Phi[..., 0], Xt[..., 0], wrapped, h, acc[:, 0], rej[:, 0], status[:, 0])
    return HaloStm(X, Phi, Xt, wrapped, h, acc, rej, status)


def stationkeep_target_gains(Phi, q=1e-2, r=None, sing_tol=1e-12, ctx=None):
    """The target-point station-keeping gains of Howell & Pernicka from phase-to-phase STMs (lto_stationkeep_target_gains_batch,
    DESIGN 4.30).  Phi [6 x 6 x K] (one record), [6 x 6 x K x P] or [6 x 6 x K x P x B], HaloStm.Phi as it is; q >= 0 the weight of
    |dv|^2, r [K] the weights of the position deviation at each target (>= 0, not all zero; default ones).  Returns
    StationkeepTargetGains(G [3 x 6 (x P (x B))] with dv = G dx = -H^-1 N dx, H = q I + sum_k r_k B_k^T B_k, N = sum_k r_k B_k^T
    [A_k | B_k]; pivot: the smallest squared Cholesky pivot of H over its largest diagonal entry; status: 0, 2 a non-finite input,
    3 a pivot not > sing_tol times the largest diagonal entry; NaN outputs where status != 0)."""
    Pp = np.asarray(Phi, dtype=np.float64)
    if Pp.ndim not in (3, 4, 5) or Pp.shape[:2] != (6, 6) or Pp.size == 0:
        raise ValueError("Phi must be [6 x 6 x K], [6 x 6 x K x P] or [6 x 6 x K x P x B]")
    K = Pp.shape[2]
    tail = Pp.shape[3:]
    q = float(q)
    if not (np.isfinite(q) and q >= 0.0):
        raise ValueError("q must be finite and >= 0")
    rr = np.ones(K) if r is None else np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1))
    if rr.size != K or not np.all(np.isfinite(rr)) or np.any(rr < 0.0) or not np.any(rr > 0.0):
        raise ValueError("r must hold one finite weight >= 0 per target, not all zero")
    sing_tol = float(sing_tol)
    if not (0.0 <= sing_tol < 1.0):
        raise ValueError("sing_tol must lie in [0, 1)")
    Pp = np.asfortranarray(Pp.reshape(6, 6, K, -1, order="F"))
    n = Pp.shape[3]
    if 36 * K * n > 0x7fffffff:
        raise ValueError("36 n_tgt n_rec must not exceed 2^31 - 1")
    ctx = ctx or default_context()
    G = np.zeros((3, 6, n), order="F")
    pivot = np.zeros(n)
    status = np.zeros(n, dtype=np.int32)
    ctx.check(ctx.fn("stationkeep_target_gains_batch")(ctx.handle, K, n, _ptr(Pp), q, _ptr(rr), sing_tol, _ptr(G), _ptr(pivot),
                                                       _ptr(status)))
    if not tail:
        return StationkeepTargetGains(G[..., 0], float(pivot[0]), int(status[0]))
    return StationkeepTargetGains(G.reshape((3, 6) + tail, order="F"), pivot.reshape(tail, order="F"), status.reshape(tail, order="F"))


AddTime = collections.namedtuple("AddTime", "XC_guess XC_out t_out tau defect status iterations history cost")
AddTimeMass = collections.namedtuple("AddTimeMass", AddTime._fields + ("propellant",))


def _indirect_add_time(entry, rows, XC, t, params, Xf_times, Xf_states, dts, n_desired, integ, flag_adjointsOnly, maxIter, solve, ctx):
    """indirect_add_time / indirect_add_time_mass: one body, `entry` the library call and `rows` its row count (None: the 12-row
    entry, which takes ndim as an argument and decides itself)."""
    if rows is not None and (np.ndim(XC) != 2 or np.shape(XC)[0] != rows):       # before any library call
        raise ValueError("%s takes one trajectory [%d x n_nodes]" % (entry, rows))
    ctx = ctx or default_context()
    integ = integ or integrator()
    X = _f64(XC)
    if X.ndim != 2:
        raise ValueError("%s takes one trajectory [ndim x n_nodes]" % entry)
    ndim, n = X.shape
    tt = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if tt.size != n:
        raise ValueError("t must have one time per node")
    dts = np.ascontiguousarray(dts, dtype=np.float64).reshape(-1)
    K = dts.size
    prm, _ = _params_array(params)
    tf = np.ascontiguousarray(Xf_times, dtype=np.float64).reshape(-1)
    ob = DirectOrbits(tf, Xf_states, tf, Xf_states)
    ob.struct.n0, ob.struct.t0, ob.struct.X0 = 0, None, None       # only the arrival side is read
    guess = np.zeros((ndim, n, K), order="F")
    t_out = np.zeros((n, K), order="F")
    tau = np.zeros(K)
    XC_out = defect = status = iters = hist = cost = prop = None
    if solve:
        XC_out = np.zeros((ndim, n, K), order="F")
        defect = np.zeros((ndim, n - 1, K), order="F")
        status = np.zeros(K, dtype=np.int32)
        iters = np.zeros(K, dtype=np.int32)
        hist = np.full((2, max(int(maxIter), 1), K), np.nan, order="F")
        cost = np.zeros(K)
        prop = np.zeros(K)
    out = lambda a: _ptr(a) if solve else None   # noqa: E731
    args = [ctx.handle]
    if rows is None:
        args.append(ndim)
    args += [n, _ptr(X), _ptr(tt), prm, C.byref(integ), C.byref(ob.struct), K, _ptr(dts), int(n_desired),
             1 if flag_adjointsOnly else 0, int(maxIter), _ptr(guess), out(XC_out), _ptr(t_out), _ptr(tau), out(defect), out(status),
             out(iters), _ptr(hist) if solve and maxIter > 0 else None, out(cost)]
    if rows is not None:
        args.append(out(prop))                                  # the mass entry's last argument
    ctx.check(ctx.fn(entry + "_batch")(*args))
    history = None
    if solve:
        history = [hist[:, ~np.isnan(hist[1, :, b]), b].T.copy() for b in range(K)]
    result = AddTime(guess, XC_out, t_out, tau, defect, status, iters, history, cost)
    return result if rows is None else AddTimeMass(*result, prop)


def indirect_add_time(XC, t, params, Xf_times, Xf_states, dts, n_desired=200, integ=None, flag_adjointsOnly=False, maxIter=10,
                      solve=True, ctx=None):
    """addTimeFinal (src/HelperFunctions.jl:196-250, re-specified: DESIGN 4.12) for K time-of-flight changes at once
    (lto_indirect_add_time_batch): the converged 12-dim solution XC [12 x n] on t [n] with a ballistic tail of dts[k] TU,
    densified at n_desired points, re-meshed onto LinRange(t[0], t[n-1] + dts[k], n) and its end snapped onto the arrival orbit
    table (Xf_times [nf] in [0, 1], Xf_states [6 x nf]); then, with solve = True, the fixed-end Newton loop on the new grids.
    Returns AddTime(XC_guess [12 x n x K], XC_out [12 x n x K], t_out [n x K], tau [K], defect [12 x (n-1) x K], status [K],
    iterations [K], history (one array of (max|defect|, alpha) per trajectory), cost [K] in DU/TU); the solve's fields are None
    when solve = False."""
    return _indirect_add_time("indirect_add_time", None, XC, t, params, Xf_times, Xf_states, dts, n_desired, integ, flag_adjointsOnly,
                              maxIter, solve, ctx)


def indirect_add_time_mass(XC, t, params, Xf_times, Xf_states, dts, n_desired=200, integ=None, flag_adjointsOnly=False, maxIter=10,
                           solve=True, ctx=None):
    """indirect_add_time for a converged solution of the 14-row variable-mass system (lto_indirect_add_time_mass_batch):
    XC [14 x n], params with Isp in the mass slot.  Rows 7..13 of the last node are zeroed on a copy; the tail of dts[k] TU is the
    14-row system's own flow with zero costates -- position and velocity coast, the costates stay exactly 0, and the mass follows
    mdot = -kappa umag(0, m) m of the same right-hand side: constant for p > 1, the full-throttle flow for p = 0, the law's idle
    flow aL / (1 + e^(1 / rho)) for p = 1.  The mass row of the guess is a starting value: with solve = True the 14-row Newton loop
    (r, v, m of the first node and r, v of the last fixed, the last node's mass costate 0) owns the final mass.  Returns
    AddTimeMass: the fields of AddTime with 14 rows -- cost [K] in DU/TU with every sample's own mass in the acceleration limit --
    plus propellant [K] = XC[6, 0] - XC_out[6, -1, k] in kg; the solve's fields are None when solve = False."""
    return _indirect_add_time("indirect_add_time_mass", 14, XC, t, params, Xf_times, Xf_states, dts, n_desired, integ, flag_adjointsOnly,
                              maxIter, solve, ctx)


Remesh = collections.namedtuple("Remesh", "XC_guess XC_out t_out defect status iterations history steps_before steps_after")


def _indirect_remesh(entry, rows, XC, t, params, n_new, weights, passes, integ, flag_adjointsOnly, maxIter, ctx, solve):
    """indirect_remesh / indirect_remesh_mass: one body, `entry` the library call and `rows` its row count (None: the 12-row entry,
    which takes ndim as an argument and decides itself)."""
    X = _f64(XC)
    if rows is not None and (X.ndim not in (2, 3) or X.shape[0] != rows):
        raise ValueError("XC must be [%d x n] or [%d x n x B]" % (rows, rows))
    ndim, n, B, batched = _batch_dims(X)
    tt, ntg = _tgrids(t, n, B)
    n_new = n if n_new is None else int(n_new)
    passes = int(passes)
    if n_new < 2:
        raise LtoError(-1, "%s: n_new must be >= 2" % entry)
    if passes < 1:
        raise LtoError(-1, "%s: passes must be >= 1" % entry)
    w = None
    if weights is not None:
        if passes != 1:
            raise LtoError(-1, "%s: caller weights are applied once: passes must be 1" % entry)
        w = _f64(weights)
        if w.shape != ((n - 1,) if not batched else (n - 1, B)):
            raise ValueError("weights must be [n_nodes - 1] or [(n_nodes - 1) x n_batch], one per old segment")
        if not np.all(np.isfinite(w)) or not np.all(w > 0.0):
            raise LtoError(-1, "%s: every weight must be finite and > 0" % entry)
    ctx = ctx or default_context()
    integ = integ or integrator()
    prm, nprm = _params_array(params)
    guess = np.zeros((ndim, n_new, B), order="F")
    t_out = np.zeros((n_new, B), order="F")
    before = np.zeros((n - 1, B), dtype=np.int32, order="F")
    after = np.zeros((n_new - 1, B), dtype=np.int32, order="F")
    XC_out = defect = status = iters = hist = None
    if solve:
        XC_out = np.zeros((ndim, n_new, B), order="F")
        defect = np.zeros((ndim, n_new - 1, B), order="F")
        status = np.zeros(B, dtype=np.int32)
        iters = np.zeros(B, dtype=np.int32)
        hist = np.full((2, max(int(maxIter), 1), B), np.nan, order="F")
    ctx.check(ctx.fn(entry + "_batch")(
        ctx.handle, *((ndim,) if rows is None else ()), n, B, _ptr(X), _ptr(tt), ntg, prm, nprm, C.byref(integ), n_new,
        _ptr(w) if w is not None else None, passes,
        1 if flag_adjointsOnly else 0, int(maxIter), _ptr(t_out), _ptr(guess), _ptr(XC_out) if solve else None,
        _ptr(defect) if solve else None, _ptr(status) if solve else None, _ptr(iters) if solve else None,
        _ptr(hist) if solve and maxIter > 0 else None, _ptr(before), _ptr(after)))
    history = None
    if solve:
        history = [hist[:, ~np.isnan(hist[1, :, b]), b].T.copy() for b in range(B)]
    if not batched:
        one = lambda a: None if a is None else a[..., 0]   # noqa: E731
        return Remesh(one(guess), one(XC_out), one(t_out), one(defect), None if status is None else int(status[0]),
                      None if iters is None else int(iters[0]), None if history is None else history[0], one(before), one(after))
    return Remesh(guess, XC_out, t_out, defect, status, iters, history, before, after)


def indirect_remesh(XC, t, params, n_new=None, weights=None, passes=2, integ=None, flag_adjointsOnly=False, maxIter=10, ctx=None,
                    solve=True):
    """Mesh re-distribution of converged 12-dim solutions (lto_indirect_remesh_batch): XC [12 x n] or [12 x n x B] on
    t [n] or [n x B] is put on n_new nodes (default n) placed so that every new segment carries the same share of a per-segment
    monitor -- weights [(n-1)] / [(n-1) x B] (then passes must be 1), or, with weights = None, the trial-step counts of a defect
    sweep with integ (adaptive integrators only), `passes` times over.  The new nodes lie on the input's own piecewise trajectory
    (XC_guess); with solve = True the Newton loop of indirect_solve_batch then runs on the new grids.  Returns Remesh(XC_guess
    [12 x n_new x B], XC_out, t_out [n_new x B], defect [12 x (n_new-1) x B], status [B], iterations [B], history, steps_before
    [(n-1) x B], steps_after [(n_new-1) x B]); a single trajectory comes back without the batch axis, the solve's fields are None
    when solve = False."""
    return _indirect_remesh("indirect_remesh", None, XC, t, params, n_new, weights, passes, integ, flag_adjointsOnly, maxIter, ctx, solve)


def indirect_remesh_mass(XC, t, params, n_new=None, weights=None, passes=2, integ=None, flag_adjointsOnly=False, maxIter=10, ctx=None,
                         solve=True):
    """indirect_remesh for converged solutions of the 14-row variable-mass system (lto_indirect_remesh_mass_batch):
    XC [14 x n] or [14 x n x B], params with Isp in the mass slot.  Monitor, grid, passes and the result object are those of
    indirect_remesh (14 rows wherever it has 12); with solve = True the 14-row Newton loop runs on the new grids: r, v and m0 of the
    first node and r, v of the last stay fixed, the final mass is free and the last node's mass costate is 0."""
    return _indirect_remesh("indirect_remesh_mass", 14, XC, t, params, n_new, weights, passes, integ, flag_adjointsOnly, maxIter, ctx,
                            solve)


def direct_qp_step_free(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, models, beta, allowImpulsive=False, ctx=None):
    """One Jacobian sweep and one FREE-END QP step (flagEnd = true, lto_direct_qp_step_free): targets (lto_direct_targets, s0 and
    sf the end states at the current tau), models (lto_direct_end_model) and beta: one, or one per trajectory.  Returns
    (x_update, u_update, dV_update[6], p[2] = (p1_update; p2_update), cost) -- with a trailing batch axis on a batched call."""
    def extra(ntgt):
        return C.cast(_end_models_array(models, ntgt), C.c_void_p), _ptr(_betas(beta, ntgt))
    return _direct_qp_call("direct_qp_step_free", 2, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, ctx, extra)


def direct_solve_free(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, orbits, targets, tau, beta, flagEnd=True, allowImpulsive=False,
                      maxIter=100, ctx=None):
    """The loop of multiShoot_CRTBP_direct with end points on the orbit tables (lto_direct_solve_free_batch): tau [2] or [2 x B] =
    (tau1; tau2) per trajectory, beta one or one per target.  The mass and impulses come from targets; s0 and sf are recomputed
    from tau.  flagEnd: free ends on odd iterations.  Returns (X_all, u_all, dV[6], t_TU, defect, tau[2], status, iterations,
    history[5 x maxIter] = (max|defect|, cost, alpha, tau1, tau2)); a trailing batch axis on X_all solves a multi-start batch."""
    def extra(ntgt, B):
        return _ptr(_taus(tau, B)), _ptr(_betas(beta, ntgt)), 1 if flagEnd else 0
    return _direct_solve_call("direct_solve_free_batch", 5, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive,
                              maxIter, ctx, orbits, extra)


def direct_tf_bounds(step, tf_min, tf_max):
    """lto_direct_tf_bounds (TU): |tf_jump| <= step per free iteration, tf_min <= tf <= tf_max (tf_min past t0)."""
    return LtoDirectTfBounds(float(step), float(tf_min), float(tf_max))


def _tf_bounds_array(tf_bounds, ntgt):
    if isinstance(tf_bounds, LtoDirectTfBounds):
        tf_bounds = [tf_bounds]
    if len(tf_bounds) != ntgt:
        raise ValueError("need as many tf bounds as targets")
    return (LtoDirectTfBounds * ntgt)(*tf_bounds)


def direct_qp_step_free_tf(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, models, beta, tf_bounds, allowImpulsive=False,
                           ctx=None):
    """One Jacobian sweep (with the tf column) and one free-end, FREE-TF QP step (lto_direct_qp_step_free_tf): as
    direct_qp_step_free, with tf_bounds (lto_direct_tf_bounds, one or one per target); tf is the last entry of each grid.  Returns
    (x_update, u_update, dV_update[6], p[3] = (p1; p2; tf_update), cost) -- with a trailing batch axis on a batched call."""
    def extra(ntgt):
        em = _end_models_array(models, ntgt)
        tb = _tf_bounds_array(tf_bounds, ntgt)
        return C.cast(em, C.c_void_p), _ptr(_betas(beta, ntgt)), C.cast(tb, C.c_void_p)
    return _direct_qp_call("direct_qp_step_free_tf", 3, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive, ctx, extra)


def direct_solve_free_tf(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, orbits, targets, tau, beta, tf_bounds, flagEnd=True,
                         allowImpulsive=False, maxIter=100, ctx=None):
    """The loop of multiShoot_CRTBP_direct with free end points AND a free time of flight (lto_direct_solve_free_tf_batch): as
    direct_solve_free, with tf_bounds (one or one per target).  Returns (X_all, u_all, dV[6], t_TU (each trajectory's final grid),
    defect, tau[2], status, iterations, history[6 x maxIter] = (max|defect|, cost, alpha, tau1, tau2, tf))."""
    def extra(ntgt, B):
        tb = _tf_bounds_array(tf_bounds, ntgt)
        return _ptr(_taus(tau, B)), _ptr(_betas(beta, ntgt)), C.cast(tb, C.c_void_p), 1 if flagEnd else 0
    return _direct_solve_call("direct_solve_free_tf_batch", 6, X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, targets, allowImpulsive,
                              maxIter, ctx, orbits, extra)


# ------------------------------------------------------------------------------------------------
# Device-resident plans (operands stay in HBM; SoA layouts of include/lto.h)
# ------------------------------------------------------------------------------------------------

def _dptr(x):
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def current_stream_ptr():
    """hipStream_t of torch's current stream (so torch events / collectives order against our launches)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class IndirectPlan:
    """lto_indirect_plan: per-trajectory parameters uploaded once, then repeated asynchronous sweeps."""

    def __init__(self, ctx, n_nodes, n_batch, params, integ, ndim=12):
        self.ctx = ctx
        self.n_nodes, self.n_batch, self.ndim = int(n_nodes), int(n_batch), int(ndim)
        self.S = (self.n_nodes - 1) * self.n_batch
        prm, nprm = _params_array(params)
        h = C.c_void_p()
        ctx.check(ctx.lib.lto_indirect_plan_create(ctx.handle, self.ndim, self.n_nodes, self.n_batch, prm, nprm,
                                                   C.byref(integ), C.byref(h)))
        self.handle = h
        ctx._plans.add(self)

    KERNEL_AUTO, KERNEL_PER_LANE, KERNEL_COOP, KERNEL_PIPE8, KERNEL_COOP2, KERNEL_PIPE48, KERNEL_PIPE32, KERNEL_LANE = 0, 1, 2, 5, 6, 7, 8, 9   # 3: LTO_KERNEL_DIRECT_PIPE (direct plans)
    KERNEL_NAMES = {0: "none yet", 1: "per-lane", 2: "cooperative", 5: "pipeline8", 6: "cooperative2", 7: "pipeline48", 8: "pipeline32", 9: "segment-lane"}

    def set_kernel(self, kernel):
        self.ctx.check(self.ctx.lib.lto_indirect_plan_set_kernel(self.handle, int(kernel)))

    LAYOUT_SOA, LAYOUT_BLOCKS = 0, 1

    def set_output_layout(self, layout):
        """LAYOUT_BLOCKS: the sweeps write defect [S][ndim] and Phi [S][ndim*ndim] (one column-major block per segment: Julia's
        layout) instead of struct-of-arrays; 12-dim DOP853 plans only (lto_indirect_plan_set_output_layout)."""
        self.ctx.check(self.ctx.lib.lto_indirect_plan_set_output_layout(self.handle, int(layout)))

    def set_defect_lanes(self, lanes=0):
        """Lanes per segment of the defect-only sweep of a 12-dim DOP853 plan: 0 = choose, 1, 2 or 4
        (lto_indirect_plan_set_defect_lanes)."""
        self.ctx.check(self.ctx.lib.lto_indirect_plan_set_defect_lanes(self.handle, int(lanes)))

    def set_warm_start(self, on=True):
        """Adaptive sweeps of this plan start every segment from its first accepted step size of the plan's previous sweep of
        the same kind (lto_indirect_plan_set_warm_start; 12-dim DOP853 plans)."""
        self.ctx.check(self.ctx.lib.lto_indirect_plan_set_warm_start(self.handle, 1 if on else 0))

    def last_kernel(self):
        """Name of the kernel family the last STM sweep ran (what AUTO resolved to)."""
        return self.KERNEL_NAMES[self.ctx.lib.lto_indirect_plan_last_kernel(self.handle)]

    def staging(self):
        """Record staging of the plan's ordered sweeps (lto_indirect_plan_staging): bit 1 node / defect records in place, bit 2 Phi records
        too (plans that run STM sweeps), bit 4 an allocation failed and staging is off."""
        return int(self.ctx.lib.lto_indirect_plan_staging(self.handle))

    def set_cols_per_lane(self, cols):
        self.ctx.check(self.ctx.lib.lto_indirect_plan_set_cols_per_lane(self.handle, int(cols)))

    def defect(self, X, ldx, t, n_tgrids, defect, ldd, errors=None, stream=None):
        self.ctx.check(self.ctx.lib.lto_indirect_defect_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t), int(n_tgrids),
                                                            _dptr(defect), int(ldd), _dptr(errors)))

    def jacobian(self, X, ldx, t, n_tgrids, Phi, ldp, defect=None, ldd=0, stream=None):
        self.ctx.check(self.ctx.lib.lto_indirect_jacobian_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t),
                                                              int(n_tgrids), _dptr(Phi), int(ldp), _dptr(defect), int(ldd)))

    def dense(self, X, ldx, t, n_tgrids, first, t_samples, Y, ldy, final_state=None, stream=None):
        """Dense output (lto_indirect_dense_dev): segment s stores its state at t_samples[first[s] : first[s+1]] into the same
        columns of Y [ndim][ldy]; first is int32 [S + 1]; final_state [ndim][n_batch], if given, takes every trajectory's x(t_n)."""
        self.ctx.check(self.ctx.lib.lto_indirect_dense_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t), int(n_tgrids),
                                                           _dptr(first), _dptr(t_samples), _dptr(Y), int(ldy), _dptr(final_state)))

    def dense_mass(self, X, ldx, t, n_tgrids, first, t_samples, Y, ldy, final_state=None, stream=None):
        """The same on a 14-row plan (lto_indirect_dense_mass_dev): X [14][ldx], Y [14][ldy], final_state [14 x n_batch] or None."""
        self.ctx.check(self.ctx.lib.lto_indirect_dense_mass_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t), int(n_tgrids),
                                                                _dptr(first), _dptr(t_samples), _dptr(Y), int(ldy), _dptr(final_state)))

    def events(self, X, ldx, t, n_tgrids, max_events, n_events, t_event, kind, on0, dv, burn_time, status, dv_seg=None, stream=None):
        """Thrust events on device arrays (lto_indirect_events_dev): n_events, kind, on0, status int32; t_event, kind
        [n_batch][max_events]; dv_seg [S] or None."""
        self.ctx.check(self.ctx.lib.lto_indirect_events_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t), int(n_tgrids),
                                                            int(max_events), _dptr(n_events), _dptr(t_event), _dptr(kind), _dptr(on0),
                                                            _dptr(dv), _dptr(burn_time), _dptr(dv_seg), _dptr(status)))

    def events_mass(self, X, ldx, t, n_tgrids, max_events, n_events, t_event, kind, on0, dv, burn_time, propellant, status,
                    dv_seg=None, dm_seg=None, stream=None):
        """The same on a 14-row plan (lto_indirect_events_mass_dev): X [14][ldx]; propellant [n_batch]; dm_seg [S] or None."""
        self.ctx.check(self.ctx.lib.lto_indirect_events_mass_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(t), int(n_tgrids),
                                                                 int(max_events), _dptr(n_events), _dptr(t_event), _dptr(kind),
                                                                 _dptr(on0), _dptr(dv), _dptr(burn_time), _dptr(dv_seg),
                                                                 _dptr(propellant), _dptr(dm_seg), _dptr(status)))

    def newton_solve(self, Phi, ldp, defect, ldd, delta, ldx, stream=None, adjoints_only=False):
        """delta = -J \\ defect on the device; Phi=None re-uses the stored factorisation (SOC re-solve)."""
        self.ctx.check(self.ctx.lib.lto_indirect_newton_solve_dev(self.handle, stream, _dptr(Phi), int(ldp), _dptr(defect),
                                                                  int(ldd), 1 if adjoints_only else 0, _dptr(delta), int(ldx)))

    def rebalance(self, stream=None):
        """Order the lanes of subsequent adaptive sweeps by the last sweep's step counts (heaviest first)."""
        self.ctx.check(self.ctx.lib.lto_indirect_plan_rebalance(self.handle, stream))

    def reset_order(self):
        self.ctx.check(self.ctx.lib.lto_indirect_plan_reset_order(self.handle))

    def copy_order(self, stream=None, out=None):
        """(kind, order): the lane order the plan's next adaptive sweep would use (lto_indirect_plan_copy_order).  kind 0: natural
        order, `order` is `out` as it was given (None if none was); 1 global, 2 windowed: order[S] int32 (written into `out` if given)."""
        if out is None:
            buf = np.full(self.S, -1, dtype=np.int32)
        else:
            buf = out
            if (not isinstance(buf, np.ndarray) or buf.dtype != np.int32 or not buf.flags["C_CONTIGUOUS"] or not buf.flags["WRITEABLE"]
                    or buf.size < self.S):
                raise LtoError(LTO_EINVAL, "copy_order: `out` must be a writeable C-contiguous int32 array of at least S = %d elements" % self.S)
        kind = C.c_int(-1)
        self.ctx.check(self.ctx.lib.lto_indirect_plan_copy_order(self.handle, stream, _ptr(buf), C.byref(kind)))
        return kind.value, (buf if (kind.value != 0 or out is not None) else None)

    def step_counts(self, stream=None):
        """(accepted[S], rejected[S]) of the last adaptive sweep (numpy int32)."""
        acc = np.zeros(self.S, dtype=np.int32)
        rej = np.zeros(self.S, dtype=np.int32)
        self.ctx.check(self.ctx.lib.lto_indirect_plan_copy_steps(self.handle, stream, _ptr(acc), _ptr(rej)))
        return acc, rej

    def steps_accepted_ptr(self):
        return self.ctx.lib.lto_indirect_plan_steps_accepted(self.handle)

    def steps_rejected_ptr(self):
        return self.ctx.lib.lto_indirect_plan_steps_rejected(self.handle)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.lto_indirect_plan_destroy(self.handle)
            self.handle = None
            self.ctx._plans.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DirectPlan:
    def __init__(self, ctx, nstate, n_nodes, n_batch, nsteps, MU, DU, TU, Isp):
        self.ctx = ctx
        self.nstate, self.n_nodes, self.n_batch, self.nsteps = int(nstate), int(n_nodes), int(n_batch), int(nsteps)
        self.S = (self.n_nodes - 1) * self.n_batch
        prm = LtoDirectParams(float(MU), float(DU), float(TU), float(Isp))
        h = C.c_void_p()
        ctx.check(ctx.lib.lto_direct_plan_create(ctx.handle, self.nstate, self.n_nodes, self.n_batch, self.nsteps,
                                                 C.byref(prm), C.byref(h)))
        self.handle = h
        ctx._plans.add(self)

    def set_kernel(self, kernel):
        self.ctx.check(self.ctx.lib.lto_direct_plan_set_kernel(self.handle, int(kernel)))

    def defect(self, X, ldx, U, ldu, t, n_tgrids, defect, ldd, errors=None, stream=None):
        self.ctx.check(self.ctx.lib.lto_direct_defect_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(U), int(ldu),
                                                          _dptr(t), int(n_tgrids), _dptr(defect), int(ldd), _dptr(errors)))

    def midpoints(self, X, ldx, U, ldu, t, n_tgrids, x_mid, ldm, defect=None, ldd=0, errors=None, stream=None):
        self.ctx.check(self.ctx.lib.lto_direct_midpoints_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(U), int(ldu),
                                                             _dptr(t), int(n_tgrids), _dptr(x_mid), int(ldm), _dptr(defect),
                                                             int(ldd), _dptr(errors)))

    def jacobian(self, X, ldx, U, ldu, t, n_tgrids, Jac, ldj, dtf=None, defect=None, ldd=0, errors=None, stream=None):
        self.ctx.check(self.ctx.lib.lto_direct_jacobian_dev(self.handle, stream, _dptr(X), int(ldx), _dptr(U), int(ldu),
                                                            _dptr(t), int(n_tgrids), _dptr(Jac), int(ldj), _dptr(dtf),
                                                            _dptr(defect), int(ldd), _dptr(errors)))

    def qp_step(self, Jac, ldj, defect, ldd, X, ldx, U, ldu, t, n_tgrids, targets, dX, dU, dV, cost, allowImpulsive=False,
                stream=None):
        """The QP step on device arrays (lto_direct_qp_step_dev): targets is a device array of n_batch lto_direct_targets (19 float64
        each: s0, sf, mass, dV1, dV2); dX [nstate][ldx], dU [3][ldu], dV [n_batch][6], cost [n_batch]."""
        self.ctx.check(self.ctx.lib.lto_direct_qp_step_dev(self.handle, stream, _dptr(Jac), int(ldj), _dptr(defect), int(ldd),
                                                           _dptr(X), int(ldx), _dptr(U), int(ldu), _dptr(t), int(n_tgrids),
                                                           _dptr(targets), 1 if allowImpulsive else 0, _dptr(dX), _dptr(dU),
                                                           _dptr(dV), _dptr(cost)))

    def costates(self, Jac, ldj, Lambda, ldl, kkt_res, mult=None, ldm=0, stream=None):
        """Costates from the multipliers of the plan's last frozen qp_step (lto_direct_costates_dev), device arrays: Lambda
        [nstate][ldl] entry b n_nodes + k, kkt_res [n_batch], mult [nstate][ldm] entry b (n_nodes - 1) + i (optional)."""
        self.ctx.check(self.ctx.lib.lto_direct_costates_dev(self.handle, stream, _dptr(Jac), int(ldj), _dptr(Lambda), int(ldl),
                                                            _dptr(mult), int(ldm), _dptr(kkt_res)))

    def qp_status_ptr(self):
        """Device int [n_batch] of the last QP step: 1 = singular KKT system (lto_direct_plan_qp_status)."""
        return self.ctx.lib.lto_direct_plan_qp_status(self.handle)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.lto_direct_plan_destroy(self.handle)
            self.handle = None
            self.ctx._plans.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_soa(ctx, aos, ndim, count, soa, ld, stream=None):
    ctx.check(ctx.lib.lto_pack_soa_dev(ctx.handle, stream, _dptr(aos), int(ndim), int(count), _dptr(soa), int(ld)))


def unpack_soa(ctx, soa, ld, ndim, count, aos, stream=None):
    ctx.check(ctx.lib.lto_unpack_soa_dev(ctx.handle, stream, _dptr(soa), int(ld), int(ndim), int(count), _dptr(aos)))


def defect_norms(ctx, defect, ldd, ndim, seg_per_traj, n_batch, sumsq, maxabs, stream=None):
    ctx.check(ctx.lib.lto_defect_norms_dev(ctx.handle, stream, _dptr(defect), int(ldd), int(ndim), int(seg_per_traj),
                                           int(n_batch), _dptr(sumsq), _dptr(maxabs)))


def trial_points(ctx, X, delta, ld, ndim, n_nodes, n_batch, alphas, Xt, ldt, stream=None):
    """Xt = the len(alphas) trial trajectories X + alpha * delta of every trajectory of the batch (device arrays; lineSearch, indirect.jl:227-233)."""
    ctx.check(ctx.lib.lto_trial_points_dev(ctx.handle, stream, _dptr(X), _dptr(delta), int(ld), int(ndim), int(n_nodes), int(n_batch),
                                           int(alphas.numel() if hasattr(alphas, "numel") else len(alphas)), _dptr(alphas), _dptr(Xt), int(ldt)))


def line_search_pick(ctx, sumsq, maxabs, alphas, trial_defect, ldt, ndim, seg_per_traj, n_batch, step, maxabs_out, defect, ldd, stream=None):
    """lineSearch's first minimiser per trajectory (indirect.jl:244-245) taken on the device: step <- alpha, maxabs_out <- the chosen trial's
    max |defect|, defect <- its defect block (the check of :328-331 without another sweep).  Device arrays."""
    na = int(alphas.numel() if hasattr(alphas, "numel") else len(alphas))
    ctx.check(ctx.lib.lto_line_search_pick_dev(ctx.handle, stream, _dptr(sumsq), _dptr(maxabs), _dptr(alphas), na, _dptr(trial_defect), int(ldt),
                                               int(ndim), int(seg_per_traj), int(n_batch), _dptr(step), _dptr(maxabs_out), _dptr(defect), int(ldd)))


def segment_order(ctx, kind, accepted, rejected, order, n_segments, weave=0, stream=None):
    """order[:n_segments] (device int32) <- the lane order of the adaptive sweeps for the step counts accepted + rejected (device
    int32): kind 1 global, 2 windowed with `weave` windows interleaved (0: the kernel's choice).  lto_segment_order_dev; back when done."""
    ctx.check(ctx.lib.lto_segment_order_dev(ctx.handle, int(kind), int(weave), int(n_segments), _dptr(accepted), _dptr(rejected),
                                            _dptr(order), stream))


def step_stats(ctx, accepted, rejected, n_segments, out=None, stream=None):
    """[sum, max, n_segments] of accepted + rejected (device int32) as k_step_stats reports them (lto_step_stats_dev): int64 [3]."""
    if out is None:
        out = np.full(3, -1, dtype=np.int64)
    if (not isinstance(out, np.ndarray) or out.dtype != np.int64 or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"] or out.size < 3):
        raise LtoError(LTO_EINVAL, "step_stats: `out` must be a writeable C-contiguous int64 array of at least 3 elements")
    ctx.check(ctx.lib.lto_step_stats_dev(ctx.handle, int(n_segments), _dptr(accepted), _dptr(rejected), _ptr(out), stream))
    return out


def read_scalars(ctx, a, na, b, nb, out, stream=None):
    """out[:na] <- device a, out[na:na+nb] <- device b (or None), back when they have arrived (lto_read_scalars_dev): the per-iteration
    read-back of a Newton loop.  `out`: a C-contiguous float64 numpy array of at least na + nb elements -- checked here, because the
    library copies na + nb doubles to the address it is given (a short or wrong-typed array would be a heap overwrite)."""
    na, nb = int(na), int(nb if b is not None else 0)
    if (not isinstance(out, np.ndarray) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]
            or na < 0 or nb < 0 or out.size < na + nb):
        raise LtoError(LTO_EINVAL, "read_scalars: `out` must be a writeable C-contiguous float64 array of at least na + nb = %d elements" % (na + nb))
    ctx.check(ctx.lib.lto_read_scalars_dev(ctx.handle, stream, _dptr(a), int(na), _dptr(b), int(nb), out.ctypes.data_as(C.c_void_p)))
    return out
