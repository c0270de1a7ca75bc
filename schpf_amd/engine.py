"""Device-resident CAVI engine: the state of scHPF._fit's loop kept in HBM.

One `DeviceCAVI` = one GPU = the count matrix (both sweep plans), the four
variational Gammas and their derived tables.  `step()` is the body of the loop at
/root/reference/schpf/scHPF_.py:657-714; `mean_negative_pois_llh()` is the default
loss (schpf/loss.py:142-168).  Nothing here computes on the CPU: it is a thin
object around the C ABI in include/schpf_hip.h.
"""
import ctypes

import numpy as np

from . import _lib

_NAMES = {"xi": _lib.XI, "theta": _lib.THETA, "eta": _lib.ETA, "beta": _lib.BETA}
_VAL_KINDS = {np.dtype(np.int32): _lib.VAL_I32, np.dtype(np.int64): _lib.VAL_I64,
              np.dtype(np.float32): _lib.VAL_F32, np.dtype(np.float64): _lib.VAL_F64}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def mean_negative(llh, gl, nnz):
    """-(sum llh) / nnz.  A matrix without stored entries has no mean: NaN, as the reference's np.mean over an empty
    array (loss.py:167) gives -- not a ZeroDivisionError."""
    return -(llh - gl) / nnz if nnz else float("nan")


def rowmean_negative(llh, gl, count):
    """-(llh - gl) / count per row, float64; NaN where a row has no stored entry (the reference's mean over an empty
    row is 0/0 = NaN too), without a warning."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -(np.asarray(llh, np.float64) - np.asarray(gl, np.float64)) / np.asarray(count, np.float64)


_AXES = {"cell": _lib.BY_CELL, "gene": _lib.BY_GENE}

ELBO_TERMS = ("data", "logfac", "rate", "cell", "gene")
PREDICTIVE_SUMS = ("zeros", "rate", "rate2")


def predicted_moments(sums, n):
    """(mean, variance, fraction of zeros) of an entry of each row from its predictive sums over n entries: given
    lambda the entry is Poisson, so its variance over the row is E[lambda] + Var[lambda] (law of total variance)."""
    mean = sums["rate"] / n
    return mean, mean + sums["rate2"] / n - mean * mean, sums["zeros"] / n


def elbo_dict(data, logfac, rate, cell, gene):
    """The five terms of the ELBO and their total, data - logfac - rate + cell + gene."""
    return {"data": data, "logfac": logfac, "rate": rate, "cell": cell, "gene": gene,
            "elbo": data - logfac - rate + cell + gene}


class DeviceCAVI(object):
    """CAVI state on one MI355X.

    Parameters
    ----------
    ncells, ngenes, nfactors : int
        ncells is the number of local cells when cells are sharded over GPUs.
    dtype : np.float64 or np.float32
        model precision (scHPF(dtype=...), scHPF_.py:239).
    device : int
        HIP device ordinal.
    stream : int or None
        a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream) to
        enqueue on; None lets the library create its own stream.  0 -- what torch
        reports for its default stream -- means the device's null stream, so that
        work torch enqueues on its current stream (collectives) is ordered with the
        engine's kernels.
    """

    def __init__(self, ncells, ngenes, nfactors, dtype=np.float64, device=0, stream=None):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.dtype = np.dtype(dtype)
        if self.dtype == np.float64:
            code = _lib.F64
        elif self.dtype == np.float32:
            code = _lib.F32
        else:
            raise TypeError("dtype must be float64 or float32")
        self.ncells, self.ngenes, self.nfactors = int(ncells), int(ngenes), int(nfactors)
        self.device = int(device)
        self.nnz = 0
        handle = ctypes.c_void_p()
        if stream is None:
            stream_arg = None
        else:
            stream_arg = int(stream) or _lib.STREAM_DEFAULT
        _lib.check(self._lib.schpf_create(ctypes.byref(handle), int(device),
                                          ctypes.c_void_p(stream_arg), code,
                                          self.ncells, self.ngenes, self.nfactors))
        self._h = handle

    # ------------------------------------------------------------------ lifetime
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.schpf_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -------------------------------------------------------------------- inputs
    def upload(self, X, warn=True):
        """X (ncells x ngenes): a SciPy sparse matrix (coo_matrix-like with .row, .col, .data, or anything with
        .tocoo()), or a torch sparse COO / CSR tensor.  A tensor in GPU memory -- it must be on this engine's device --
        is handed to the library by pointer and validated, converted and planned there: nothing of it
        crosses PCIe, and the engine ends up as after an upload of the same entries from the host.  A CPU tensor takes
        the host path.  warn=False: the caller issues rounding_warning() itself (a helper thread must not touch the
        warnings machinery)."""
        from .device_input import classify
        inp = classify(X, (self.ncells, self.ngenes))
        if inp.kind == "host":
            X = inp.matrix
            data = np.ascontiguousarray(X.data)
            if data.dtype not in _VAL_KINDS:
                data = data.astype(np.float64)
            row = np.ascontiguousarray(X.row, dtype=np.int32)
            col = np.ascontiguousarray(X.col, dtype=np.int32)
            _lib.check(self._lib.schpf_upload_coo(self._h, data.shape[0], _p(row), _p(col), _p(data),
                                                  _VAL_KINDS[data.dtype]))
        else:
            import torch
            if inp.device != self.device:
                raise ValueError("X is on GPU %d, the engine on GPU %d" % (inp.device, self.device))
            torch.cuda.current_stream(inp.device).synchronize()     # whatever produced X has finished
            ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
            if inp.kind == "coo":
                status = self._lib.schpf_upload_coo_device(self._h, inp.nnz, ptr(inp.major), ptr(inp.minor),
                                                           inp.minor_kind, ptr(inp.values), inp.value_kind)
            else:
                status = self._lib.schpf_upload_csr_device(self._h, inp.nnz, ptr(inp.major), inp.major_kind,
                                                           ptr(inp.minor), inp.minor_kind, ptr(inp.values),
                                                           inp.value_kind)
            _lib.check(status)
        self.nnz = inp.nnz
        if warn:
            self.rounding_warning(stacklevel=3)

    def marginals(self):
        """(row_sums, col_sums) of the matrix the engine holds, float64 [ncells] / [ngenes]: what X.sum(1) / X.sum(0)
        give, from the sums the engine keeps anyway (exact for counts).  A batch engine (upload_rows) raises."""
        rows, cols = np.empty(self.ncells, np.float64), np.empty(self.ngenes, np.float64)
        _lib.check(self._lib.schpf_marginals(self._h, rows.ctypes.data_as(_lib._dblp), cols.ctypes.data_as(_lib._dblp)))
        return rows, cols

    def rounding_warning(self, stacklevel=2):
        """Warn (on the calling thread) if the last upload rounded values of X.data to float32."""
        info = self.upload_info()
        if info["rounded"]:
            import warnings
            warnings.warn("%d of %d values of X.data are not exactly representable in float32 and were "
                          "rounded (relative error <= 6e-8); counts are stored as float32 on the device"
                          % (info["rounded"], info["nnz"]), RuntimeWarning, stacklevel=stacklevel)

    def keep_rows(self, on=True):
        """Call before upload(): also keep a row-sorted copy of the matrix in HBM, from which batch
        engines gather their rows (upload_rows) -- minibatch CAVI without host slicing or re-uploads."""
        _lib.check(self._lib.schpf_keep_rows(self._h, int(bool(on))))

    def upload_rows(self, source, rows):
        """This engine's matrix := rows `rows` (in that order) of `source`'s matrix (a DeviceCAVI on the
        same device that was told to keep_rows()); len(rows) must be this engine's ncells."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        _lib.check(self._lib.schpf_upload_rows(self._h, source._h, _p(rows), int(rows.shape[0])))
        self.nnz = self.upload_info()["nnz"]

    def upload_info(self):
        """{'nnz', 'rounded' (values rounded to float32), 'zeros' (explicitly stored), 'packed', 'rows'
        (a row-sorted copy is resident: keep_rows() took effect -- device-built tile plans only)}."""
        info = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.schpf_upload_info(self._h, info))
        out = dict(zip(("nnz", "rounded", "zeros"), [int(v) for v in info[:3]]))
        out["packed"], out["rows"] = int(info[3]) & 1, bool(int(info[3]) & 2)
        return out

    def set_hypers(self, a, c, bp, dp):
        _lib.check(self._lib.schpf_set_hypers(self._h, float(a), float(c), float(bp), float(dp)))

    def _dims(self, name):
        n = self.ncells if name in ("xi", "theta") else self.ngenes
        return (n, self.nfactors) if name in ("theta", "beta") else (n,)

    def _torch_dtype(self):
        import torch
        return torch.float64 if self.dtype == np.float64 else torch.float32

    def set_gamma(self, name, vi_shape, vi_rate):
        """vi_shape / vi_rate: array-likes (converted to the engine's dtype), or two torch tensors on the engine's GPU of
        the engine's dtype, which are copied device to device."""
        from .device_input import on_gpu
        dims = self._dims(name)
        if on_gpu(vi_shape) or on_gpu(vi_rate):
            s, r = vi_shape, vi_rate
            for t in (s, r):
                if not on_gpu(t) or t.device.index != self.device or t.dtype != self._torch_dtype():
                    raise ValueError("%s must be two %s tensors on GPU %d" % (name, self._torch_dtype(), self.device))
                if tuple(t.shape) != dims:
                    raise ValueError("%s must have shape %s, got %s" % (name, dims, tuple(t.shape)))
            import torch
            s, r = s.contiguous(), r.contiguous()
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self._lib.schpf_set_state_device(self._h, _NAMES[name], ctypes.c_void_p(s.data_ptr()),
                                                        ctypes.c_void_p(r.data_ptr())))
            return
        s = np.ascontiguousarray(vi_shape, dtype=self.dtype)
        r = np.ascontiguousarray(vi_rate, dtype=self.dtype)
        if s.shape != dims or r.shape != dims:
            raise ValueError("%s must have shape %s, got %s / %s" % (name, dims, s.shape, r.shape))
        _lib.check(self._lib.schpf_set_state(self._h, _NAMES[name], _p(s), _p(r)))

    def get_gamma(self, name, device=False):
        """(vi_shape, vi_rate) as NumPy arrays; device=True: as torch tensors on the engine's GPU (a device-to-device
        copy, nothing crosses PCIe)."""
        dims = self._dims(name)
        if device:
            import torch
            s = torch.empty(dims, dtype=self._torch_dtype(), device="cuda:%d" % self.device)
            r = torch.empty_like(s)
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self._lib.schpf_get_state_device(self._h, _NAMES[name], ctypes.c_void_p(s.data_ptr()),
                                                        ctypes.c_void_p(r.data_ptr())))
            return s, r
        s = np.empty(dims, dtype=self.dtype)
        r = np.empty(dims, dtype=self.dtype)
        _lib.check(self._lib.schpf_get_state(self._h, _NAMES[name], _p(s), _p(r)))
        return s, r

    # ----------------------------------------------------------------- iteration
    def init_phi_host(self, Xphi_data):
        """t == 0 responsibilities drawn by the caller (scHPF_.py:652-655)."""
        x = np.ascontiguousarray(Xphi_data, dtype=np.float64)
        if x.shape != (self.nnz, self.nfactors):
            raise ValueError("Xphi_data must be (nnz, nfactors)")
        _lib.check(self._lib.schpf_init_phi_host(self._h, _p(x)))

    def init_phi_device(self, seed):
        _lib.check(self._lib.schpf_init_phi_device(self._h, ctypes.c_uint64(int(seed) & (2 ** 64 - 1))))

    @staticmethod
    def _flags(freeze_genes, simultaneous, sharded=False, cells_first=False):
        return ((_lib.FREEZE_GENES if freeze_genes else 0) | (_lib.SIMULTANEOUS if simultaneous else 0)
                | (_lib.SHARDED if sharded else 0) | (_lib.CELLS_FIRST if cells_first else 0))

    def step(self, freeze_genes=False, simultaneous=False, cells_first=False):
        """One CAVI iteration.  cells_first=True is the reference's minibatch order
        (scHPF_.py:688-704): cell block from the current beta, then gene block from the new theta."""
        _lib.check(self._lib.schpf_step(self._h, self._flags(freeze_genes, simultaneous,
                                                             cells_first=cells_first)))

    def steps(self, n, freeze_genes=False, simultaneous=False, cells_first=False):
        """n CAVI iterations in one call (the stretch between two loss checks); replayed as one
        hipGraph from the second call with the same arguments."""
        _lib.check(self._lib.schpf_steps(self._h, self._flags(freeze_genes, simultaneous,
                                                              cells_first=cells_first), int(n)))

    def step_local(self, freeze_genes=False, simultaneous=False, side=None):
        """Sweeps of the sharded iteration.  side=None: both; 'gene': the gene-side sweep and the
        packing of its sums into the exchange buffer; 'cell': the cell-side sweep (so that the
        caller can overlap it with the all-reduce of the gene-side sums)."""
        extra = {None: 0, "gene": _lib.LOCAL_GENE, "cell": _lib.LOCAL_CELL}[side]
        _lib.check(self._lib.schpf_step_local(self._h, self._flags(freeze_genes, simultaneous, True) | extra))

    def step_finish(self, freeze_genes=False, simultaneous=False):
        _lib.check(self._lib.schpf_step_finish(self._h, self._flags(freeze_genes, simultaneous, True)))

    # ------------------------------------------------- sharded, collective inside the library
    @staticmethod
    def comm_unique_id():
        """128 bytes identifying a new RCCL communicator: generate on ONE rank, give to all."""
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().schpf_comm_unique_id(buf))
        return buf.raw

    def hint_sharded(self, on=True):
        """Call before upload() when the engine will run sharded iterations (two sweep launches)."""
        _lib.check(self._lib.schpf_hint_sharded(self._h, int(bool(on))))

    def hint_transient(self, on=True):
        """Call before upload() when the engine's matrix will be replaced every iteration (minibatches sliced on the
        host): its plans are then built the cheapest way (no balancing pass)."""
        _lib.check(self._lib.schpf_hint_transient(self._h, int(bool(on))))

    def comm_init(self, unique_id, rank, world):
        """Join the communicator (collective: returns once all `world` ranks have called it)."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        try:
            _lib.check(self._lib.schpf_comm_init(self._h, ctypes.c_char_p(bytes(unique_id)), int(rank), int(world)))
        except _lib.SchpfHipError as e:
            raise _lib.SchpfHipError(str(e) + _lib.ipc_hint())
        self.comm_world = int(world)

    def comm_destroy(self):
        """Leave the communicator (captured stretches that hold its all-reduce are dropped first)."""
        _lib.check(self._lib.schpf_comm_destroy(self._h))
        self.comm_world = 0

    def steps_sharded(self, n, freeze_genes=False, simultaneous=False):
        """n iterations of the sharded protocol with the all-reduce issued by the library."""
        _lib.check(self._lib.schpf_steps_sharded(self._h, self._flags(freeze_genes, simultaneous), int(n)))

    def loss_terms_all(self):
        llh, gl, nnz = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(self._lib.schpf_loss_terms_all(self._h, ctypes.byref(llh), ctypes.byref(gl), ctypes.byref(nnz)))
        return llh.value, gl.value, nnz.value

    def exchange_buffer(self):
        """(device pointer, element count) of the buffer to all-reduce between
        step_local and step_finish; elements have the model dtype."""
        ptr, count = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(self._lib.schpf_exchange_buffer(self._h, ctypes.byref(ptr), ctypes.byref(count)))
        return ptr.value, count.value

    def loss_terms(self):
        """(sum x log r - r, sum lgamma(x+1), nnz) over the local nonzeros."""
        llh, gl, nnz = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(self._lib.schpf_loss_terms(self._h, ctypes.byref(llh), ctypes.byref(gl), ctypes.byref(nnz)))
        return llh.value, gl.value, nnz.value

    def mean_negative_pois_llh(self):
        llh, gl, nnz = self.loss_terms()
        return mean_negative(llh, gl, nnz)

    def loss_rows(self, by="cell"):
        """Per cell (by="cell") or per gene (by="gene"), over the local stored entries of that row -- duplicates are
        separate observations, stored zeros count --: (sum x log r - r, sum lgamma(x+1), number of entries), float64,
        float64 and int64 arrays of ncells / ngenes.  One sweep of the plan of that axis on the device;
        the state is only read, and two calls on one state return the same bits."""
        if by not in _AXES:
            raise ValueError("by must be 'cell' or 'gene', got %r" % (by,))
        n = self.ncells if by == "cell" else self.ngenes
        llh, gl, cnt = np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.int64)
        _lib.check(self._lib.schpf_loss_rows(self._h, _AXES[by], llh.ctypes.data_as(_lib._dblp),
                                             gl.ctypes.data_as(_lib._dblp), cnt.ctypes.data_as(_lib._i64p)))
        return llh, gl, cnt

    def cellmean_negative_pois_llh(self):
        """Mean negative Poisson log-likelihood of each cell's stored entries (NaN for a cell without any)."""
        return rowmean_negative(*self.loss_rows("cell"))

    def genemean_negative_pois_llh(self):
        """Mean negative Poisson log-likelihood of each gene's stored entries (NaN for a gene without any)."""
        return rowmean_negative(*self.loss_rows("gene"))

    def predictive_rows(self, by="gene", which=PREDICTIVE_SUMS):
        """Posterior predictive sums of the state the engine holds: per cell (by="cell") or per gene
        (by="gene"), over ALL rows m of the other axis, with lambda = E[theta] . E[beta]: {"zeros": sum exp(-lambda),
        "rate": sum lambda, "rate2": sum lambda^2}, float64 arrays of ncells / ngenes.  No matrix need be uploaded; the
        state is only read, and two calls on one state return the same bits.  `which`: the sums wanted (the others are
        not copied back)."""
        if by in _AXES:
            code = _AXES[by]
        elif isinstance(by, int) and not isinstance(by, bool):
            code = by       # an axis code of the C ABI; the library refuses what it does not know
        else:
            raise ValueError("by must be 'cell' or 'gene', got %r" % (by,))
        unknown = [w for w in which if w not in PREDICTIVE_SUMS]
        if unknown:
            raise ValueError("which must be drawn from %s, got %r" % (PREDICTIVE_SUMS, unknown))
        n = self.ngenes if code == _lib.BY_GENE else self.ncells
        out = {w: np.empty(n, np.float64) for w in PREDICTIVE_SUMS if w in which}
        ptr = [out[w].ctypes.data_as(_lib._dblp) if w in out else None for w in PREDICTIVE_SUMS]
        _lib.check(self._lib.schpf_predictive_rows(self._h, code, *ptr))
        return out

    def elbo_terms(self, ap, cp):
        """The evidence lower bound of the current state over the local cells, by term:
        {'data', 'logfac', 'rate', 'cell', 'gene', 'elbo'}, elbo = data - logfac - rate + cell + gene.
        ap, cp: the shape priors of xi / eta (a, c, bp, dp are the engine's, set_hypers)."""
        t = (ctypes.c_double * 5)()
        _lib.check(self._lib.schpf_elbo_terms(self._h, float(ap), float(cp), t))
        return elbo_dict(*t)

    def elbo(self, ap, cp):
        return self.elbo_terms(ap, cp)["elbo"]

    def _debug_tables(self, by):
        """Test hook: the tables the sweeps read for one side (by="cell": theta's, by="gene": beta's), as three
        (n, KP) arrays of the engine's dtype, padding columns k >= nfactors included: {'e': shape / rate,
        'log': psi(shape) - log(rate), 'exp': exp(log - float32(row max of log))}.  Tables older than the parameters are
        rebuilt first, as the next step() or loss_terms() would; nothing else changes."""
        if by not in _AXES:
            raise ValueError("by must be 'cell' or 'gene', got %r" % (by,))
        n = self.ncells if by == "cell" else self.ngenes
        out = {k: np.empty((n, self.plan_info()["KP"]), dtype=self.dtype) for k in ("e", "log", "exp")}
        _lib.check(self._lib.schpf_debug_tables(self._h, _AXES[by], _p(out["e"]), _p(out["log"]), _p(out["exp"])))
        return out

    def synchronize(self):
        _lib.check(self._lib.schpf_synchronize(self._h))

    def stream_handle(self):
        """The hipStream_t (as an int; 0 = null stream) the engine enqueues on."""
        h = ctypes.c_void_p()
        _lib.check(self._lib.schpf_stream_handle(self._h, ctypes.byref(h)))
        return h.value or 0

    # ----------------------------------------------------------------- reporting
    def profile(self, enable=True):
        _lib.check(self._lib.schpf_profile_enable(self._h, int(bool(enable))))

    def profile_read(self):
        ms = (ctypes.c_double * 4)()
        n = (ctypes.c_int64 * 4)()
        _lib.check(self._lib.schpf_profile_read(self._h, ms, n))
        keys = ("cell_sweep", "gene_sweep", "loss_sweep", "gamma_updates")
        return {k: {"ms": ms[i], "launches": n[i]} for i, k in enumerate(keys)}

    def profile_clock(self):
        """(MHz, launches): the shader clock the device sustained under the sweep launches since the last call."""
        mhz, n = ctypes.c_double(), ctypes.c_int64()
        _lib.check(self._lib.schpf_profile_clock(self._h, ctypes.byref(mhz), ctypes.byref(n)))
        return mhz.value, n.value

    def sweep_bytes(self):
        """Bytes one iteration moves through the LDS / streams from HBM, from the tile plans (zeros otherwise)."""
        info = (ctypes.c_int64 * 8)()
        _lib.check(self._lib.schpf_sweep_bytes(self._h, info))
        keys = ("lds_read_nonzeros", "lds_read_stored_slots", "lds_staged_cell", "lds_staged_gene",
                "hbm_entry_stream", "partial_rows", "loss_side", "loss_tasks")
        return dict(zip(keys, [int(v) for v in info]))

    def plan_info(self):
        info = (ctypes.c_int64 * 16)()
        _lib.check(self._lib.schpf_plan_info(self._h, info))
        keys = ("KP", "KL", "LPC", "chunk_len", "windows_cell", "windows_gene", "n_chunks_cell",
                "n_chunks_gene", "n_waves_cell", "n_waves_gene", "entry_slots_cell", "entry_slots_gene",
                "ring_cell", "ring_gene", "ring_slot_bytes", "waves_per_block")
        return dict(zip(keys, [int(v) for v in info]))
