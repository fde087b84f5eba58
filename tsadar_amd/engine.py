"""Engine: builds the static ``tsff_config`` from a tsadar input deck and drives libtsff.so.

Device memory is held in torch CUDA tensors (torch is plumbing here: allocation, streams,
torch.distributed); every compute step is a HIP kernel inside libtsff.so reached through the C ABI.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import _lib as L
from . import distribution as D
from .params import SlotMap

_HERE = os.path.dirname(os.path.abspath(__file__))
_DATA = os.path.join(_HERE, "data")

C_LIGHT = 2.99792458e10


def xi_grids():
    """form_factor.py:128-138."""
    minmax, h1 = 8.2, 1024
    xi1 = np.linspace(-minmax - np.sqrt(2.0) / h1, minmax + np.sqrt(2.0) / h1, h1)
    xi2 = np.arange(-minmax, minmax, 0.01)
    return xi1, xi2


def zprime_tables(xi2):
    """form_factor.py:20-45 restricted to |xi| <= 10: linear interpolation of the shipped tables."""
    rd = np.loadtxt(os.path.join(_DATA, "rdWT.txt"))
    im = np.loadtxt(os.path.join(_DATA, "idWT.txt"))
    return np.interp(xi2, rd[:, 0], rd[:, 1]), np.interp(xi2, im[:, 0], im[:, 1])


def log_ratio_table(xi1, xi2):
    """Lg[q][i] = log|(gav + gdif/2) / (gav - gdif/2)| of ratintn.ratcen (ratintn.py:41-49) for
    g = xi1 - xi2[q], i = 0..1021 (the last interval is dropped, :21), zero-padded to 1024 columns.
    With it the Re(chi_e) table of a distribution function is two matrix-vector products."""
    g = xi1[None, :] - xi2[:, None]
    gdif = g[:, 1:-1] - g[:, 0:-2]
    gav = 0.5 * (g[:, 1:-1] + g[:, 0:-2])
    assert np.all(np.abs(gdif) >= 1.0e-4 * np.abs(gav)), "ratcen's small-gdif branch would trigger"
    out = np.zeros((xi2.size, xi1.size))
    out[:, : xi1.size - 2] = np.log(np.abs((gav + 0.5 * gdif) / (gav - 0.5 * gdif)))
    return out


def wavelength_axis_nm(lam_range, npts):
    """The axis the reference hands to the IRF: lamAxis = squeeze(2 pi c / omgs) * 1e7
    (form_factor.py:132-135, 293; generate_spectra.py:163, 191)."""
    lam = np.linspace(lam_range[0], lam_range[1], npts)
    omgs = 2e7 * np.pi * C_LIGHT / lam
    return (2 * np.pi * C_LIGHT / omgs) * 1e7


def gaussian_taps(lam_nm, stddev, cutoff_sigmas):
    """Taps of ``jnp.convolve(x, g, "same")`` with g the Gaussian of irf.py:66-72 / 110-114 sampled
    on the full wavelength axis: y[j] = sum_d g[c + d] x[j - d], c = (n - 1) // 2.  Taps further than
    ``cutoff_sigmas`` standard deviations from the origin are dropped (their relative weight is
    below exp(-cutoff^2 / 2)); ``cutoff_sigmas <= 0`` keeps every non-zero tap."""
    n = lam_nm.size
    origin = (np.amax(lam_nm) + np.amin(lam_nm)) / 2.0
    g = (1.0 / (stddev * np.sqrt(2.0 * np.pi))) * np.exp(-((lam_nm - origin) ** 2.0) / (2.0 * stddev**2.0))
    c = (n - 1) // 2
    if cutoff_sigmas and cutoff_sigmas > 0:
        keep = np.nonzero(np.abs(lam_nm - origin) <= cutoff_sigmas * stddev)[0]
    else:
        keep = np.nonzero(g > 0)[0]
    lo, hi = int(keep[0]), int(keep[-1])
    return np.ascontiguousarray(g[lo : hi + 1]), lo - c


def binned_taps(g, dmin, ppp):
    """Fold the ppp-sample bin average (irf.py:74,124) into the taps of ``gaussian_taps``:
    ybin[p] = (1/ppp) sum_jj y[p ppp + jj],  y[j] = sum_d g[d] x[j - d]  ==>  ybin[p] = sum_s hb[s] x[p ppp + off + s]
    with hb[s] = (1/ppp) sum_jj g[jj - s + nt - 1] and off = -(dmin + nt - 1)."""
    nt = g.size
    hb = np.zeros(nt + ppp - 1)
    for jj in range(ppp):
        # s = jj - t + nt - 1 for t = 0..nt-1
        hb[jj : jj + nt] += g[::-1]
    return np.ascontiguousarray(hb / ppp), -(dmin + nt - 1)


def _as_c(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    ptr_t = L.c_double_p if dtype == np.float64 else L.c_uint8_p
    return a, a.ctypes.data_as(ptr_t)


class Engine:
    """One libtsff handle for one (deck, scattering angles) pair on the current CUDA/HIP device."""

    def __init__(self, cfg: Dict, scattering_angles: Dict, activate: bool = True, fe_shared: Optional[np.ndarray] = None,
                 fe_mode: Optional[int] = None, irf_cutoff_sigmas: float = 12.0, irf_allow_cut: bool = True):
        import torch

        if not torch.cuda.is_available():
            raise L.TsffError("tsadar_amd needs a HIP device (no CPU fallback)")
        self.torch = torch
        self.lib = L.load()
        self.cfg = cfg
        other, data = cfg["other"], cfg["data"]
        ext = other["extraoptions"]
        self.slots = SlotMap(cfg["parameters"], activate)
        sm = self.slots
        self.n_ion, self.NP = sm.n_ion, sm.NP
        self.npts = int(other["npts"])
        self.load_ele, self.load_ion = bool(ext["load_ele_spec"]), bool(ext["load_ion_spec"])
        if other.get("iawoff", 0):
            raise NotImplementedError("iawoff cannot run under vmap in the reference (generate_spectra.py:199-208)")
        gen = cfg["parameters"]["general"]
        assert gen["Te_gradient"]["num_grad_points"] == gen["ne_gradient"]["num_grad_points"], \
            "Number of gradient points for Te and ne must be the same"  # generate_spectra.py:70-73
        fecfg = cfg["parameters"]["electron"]["fe"]
        self.fe_dim = int(fecfg.get("dim", 1))
        if self.fe_dim not in (1, 2):
            raise NotImplementedError(f"Not implemented distribution dimension: {self.fe_dim}")  # ts_params.py:164
        if self.fe_dim == 2 and fe_mode is None:
            fe_mode = L.FE_PER_LINEOUT  # the 1-D tables are unused: only form_factor_2d / ats_spectrum run
        self.nvx = int(fecfg["nvx"])

        c = L.TsffConfig()
        keep = []  # numpy arrays referenced by the struct
        c.abi_version = L.ABI_VERSION
        c.lamrangE[:] = [float(v) for v in other["lamrangE"]]
        c.lamrangI[:] = [float(v) for v in other["lamrangI"]]
        c.npts = self.npts
        c.load_ele, c.load_ion = int(self.load_ele), int(self.load_ion)
        c.ele_lam_shift = float(data.get("ele_lam_shift", 0.0))
        sa = np.asarray(scattering_angles["sa"], dtype=np.float64)
        w0 = np.asarray(scattering_angles["weights"])[0]  # generate_spectra.py:165,197
        w = np.broadcast_to(np.asarray(w0, dtype=np.float64), sa.shape)
        c.n_angles = sa.size
        a, c.sa_deg = _as_c(sa, np.float64); keep.append(a)
        a, c.sa_weights = _as_c(w, np.float64); keep.append(a)
        c.num_grad_points = int(gen["Te_gradient"]["num_grad_points"])
        c.n_ion = sm.n_ion
        c.nvx = self.nvx

        # distribution function mode
        if fe_mode is None:
            if fe_shared is not None:
                fe_mode = L.FE_SHARED
            elif sm.fe_type == "dlm":
                fe_mode = L.FE_DLM if fecfg.get("active", False) else L.FE_SHARED
            else:
                fe_mode = L.FE_PER_LINEOUT
        self.fe_mode = fe_mode
        c.fe_mode = fe_mode
        if fe_mode == L.FE_SHARED:
            if fe_shared is None:
                if sm.fe_type != "dlm":
                    raise NotImplementedError(f"Unknown 1D distribution type: {fecfg['type']}")
                fe_shared = D.dlm(float(fecfg["params"]["m"]["val"]), self.nvx)
            a, c.fe_shared = _as_c(fe_shared, np.float64); keep.append(a)
            self.fe_shared = a
        if fe_mode == L.FE_DLM:
            a, c.dlm_table = _as_c(D.dlm_table(self.nvx), np.float64); keep.append(a)

        xi1, xi2 = xi_grids()
        assert xi1.size == L.NXI1 and xi2.size == L.NXI2
        zr, zi = zprime_tables(xi2)
        for name, arr in (("xi1", xi1), ("xi2", xi2), ("zprime_re", zr), ("zprime_im", zi)):
            a, p = _as_c(arr, np.float64); keep.append(a); setattr(c, name, p)
        if fe_mode != L.FE_SHARED:
            a, c.lg_table = _as_c(log_ratio_table(xi1, xi2), np.float64); keep.append(a)

        # instrument response
        phys = other["PhysParams"]
        c.norm = int(phys["norm"])
        lamE = wavelength_axis_nm(other["lamrangE"], self.npts)
        lamI = wavelength_axis_nm(other["lamrangI"], self.npts)
        def set_taps(cutoff):
            if self.load_ele:
                t, d0 = gaussian_taps(lamE, float(phys["widIRF"]["spect_stddev_ele"]), cutoff)
                t, off = binned_taps(t, d0, self.npts // L.NBINS)
                a, c.taps_ele = _as_c(t, np.float64); keep.append(a)
                c.n_taps_ele, c.tap_off_ele = t.size, off
            if self.load_ion and phys["widIRF"]["spect_stddev_ion"]:
                t, d0 = gaussian_taps(lamI, float(phys["widIRF"]["spect_stddev_ion"]), cutoff)
                t, off = binned_taps(t, d0, self.npts // L.NBINS)
                a, c.taps_ion = _as_c(t, np.float64); keep.append(a)
                c.n_taps_ion, c.tap_off_ion = t.size, off

        set_taps(irf_cutoff_sigmas)
        filt = other.get("iawfilter", [0, 0, 0, 0])
        if self.load_ele and filt[0]:
            fb, fr = filt[3] - filt[2] / 2, filt[3] + filt[2] / 2
            if other["lamrangE"][0] < fr and other["lamrangE"][1] > fb:
                mult = np.where((fb < lamE) & (fr > lamE), 10.0 ** (-filt[1]), 1.0)
                a, c.ele_filter = _as_c(mult, np.float64); keep.append(a)

        # parameter transform
        a, c.p_scale = _as_c(sm.scale, np.float64); keep.append(a)
        a, c.p_shift = _as_c(sm.shift, np.float64); keep.append(a)
        a, c.p_sigmoid = _as_c(sm.sigmoid, np.uint8); keep.append(a)
        c.ti_same[:] = [int(v) for v in sm.ti_same]

        # loss masks on the binned axes (loss_function.py:224-259)
        method = cfg.get("optimizer", {}).get("loss_method", "l2")
        if method not in L.LOSS_METHODS:
            raise NotImplementedError(f"loss_method {method}")
        c.loss_method = L.LOSS_METHODS[method]
        ppp = self.npts // L.NBINS
        self.lamE_bin = lamE.reshape(L.NBINS, ppp).mean(axis=1)
        self.lamI_bin = lamI.reshape(L.NBINS, ppp).mean(axis=1)
        r = data["fit_rng"]
        mE = np.zeros(L.NBINS, dtype=np.uint8)
        mI = np.zeros(L.NBINS, dtype=np.uint8)
        if ext.get("fit_EPWb", False):
            mE |= ((self.lamE_bin > r["blue_min"]) & (self.lamE_bin < r["blue_max"])).astype(np.uint8)
        if ext.get("fit_EPWr", False):
            mE |= (((self.lamE_bin > r["red_min"]) & (self.lamE_bin < r["red_max"])).astype(np.uint8) << 1)
        if ext.get("fit_IAW", False):
            mI |= (((self.lamI_bin > r["iaw_min"]) & (self.lamI_bin < r["iaw_cf_min"]))
                   | ((self.lamI_bin > r["iaw_cf_max"]) & (self.lamI_bin < r["iaw_max"]))).astype(np.uint8)
        self.mask_ele, self.mask_ion = mE, mI
        a, c.mask_ele = _as_c(mE, np.uint8); keep.append(a)
        a, c.mask_ion = _as_c(mI, np.uint8); keep.append(a)
        self.n_blue = int(np.count_nonzero(mE & 1))
        self.n_red = int(np.count_nonzero(mE & 2))
        self.n_iaw = int(np.count_nonzero(mI & 1))
        self.fit_blue, self.fit_red, self.fit_iaw = bool(ext.get("fit_EPWb")), bool(ext.get("fit_EPWr")), bool(ext.get("fit_IAW"))

        self._keep = keep
        self._staging = {}
        self._last_stream = None
        self._cfg_struct = c
        h = C.c_void_p()
        cutoff = irf_cutoff_sigmas
        while True:
            rc = self.lib.tsff_create(C.byref(c), C.byref(h))
            msg = self.lib.tsff_last_error(None) if rc else b""
            # Wide instrument functions at several points per pixel: spectrum + halo + taps outgrow the LDS of a CU.  The taps
            # beyond ~8 sigma only matter below 1e-14 of a spectrum's maximum (they reproduce the reference's full-length
            # convolution in the 1e-22 tails): drop them step by step down to 7 sigma (2e-11) before giving up, and say so.
            # ``irf_allow_cut=False`` makes the overflow an error instead; the cut-off actually used is ``self.irf_cutoff_sigmas``.
            if rc == L.ERR_LDS and irf_allow_cut and cutoff and cutoff > 7.0:
                cutoff = max(7.0, cutoff - 1.0)
                set_taps(cutoff)
                continue
            break
        L.check(self.lib, None, rc)
        if cutoff != irf_cutoff_sigmas:
            import warnings
            warnings.warn(f"tsadar_amd: IRF taps cut at {cutoff} sigma instead of {irf_cutoff_sigmas} to fit the LDS "
                          f"(relative weight of the dropped taps below {np.exp(-0.5 * cutoff ** 2):.1e})")
        self.irf_cutoff_sigmas = cutoff
        self.h = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        # axes as the library computed them
        ae, ai = np.zeros(L.NBINS), np.zeros(L.NBINS)
        L.check(self.lib, self.h, self.lib.tsff_get_axes(self.h, ae.ctypes.data_as(L.c_double_p), ai.ctypes.data_as(L.c_double_p)))
        self.lamAxisE, self.lamAxisI = ae, ai

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            self.lib.tsff_destroy(h)
            self.h = None

    # ---- helpers ------------------------------------------------------------------------------
    def dev(self, a, dtype=None):
        """numpy / torch -> contiguous float64 CUDA tensor on this engine's device (no copy if it
        already is one)."""
        torch = self.torch
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            t = a
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        return t.to(device=self.device, dtype=dtype or torch.float64).contiguous()

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)

    # ---- host <-> device staging of the per-step vectors (pinned buffers: a fit step moves ~0.5 MB in and ~0.2 MB out) ----
    def upload(self, a: np.ndarray):
        """NumPy array -> device tensor through a persistent pinned staging buffer (asynchronous copy on the current stream).
        One device tensor per array SHAPE: the result aliases the previous upload of the same shape (a fit step consumes
        its parameters before the next step uploads new ones); copy it if it must outlive the next call.  The pinned buffer is
        not rewritten before its previous copy has completed (event per buffer)."""
        torch = self.torch
        a = np.ascontiguousarray(a, dtype=np.float64)
        key = ("in", a.shape)
        buf = self._staging.get(key)
        if buf is None:
            buf = (torch.empty(a.shape, dtype=torch.float64).pin_memory(), torch.empty(a.shape, dtype=torch.float64, device=self.device),
                   torch.cuda.Event())
            self._staging[key] = buf
        else:
            buf[2].synchronize()   # (the earlier H2D copy out of this pinned buffer)
        pin, dev, ev = buf
        pin.numpy()[...] = a
        self._follow_stream()   # (the device tensor may still be read by the previous call on another stream)
        dev.copy_(pin, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        return dev

    def download(self, t) -> np.ndarray:
        """Device tensor -> NumPy (pinned staging, one synchronisation of the current stream)."""
        torch = self.torch
        key = ("out", tuple(t.shape))
        pin = self._staging.get(key)
        if pin is None:
            pin = torch.empty(tuple(t.shape), dtype=t.dtype).pin_memory()
            self._staging[key] = pin
        pin.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return pin.numpy().copy()

    def _follow_stream(self):
        """torch's current stream, made to wait for the stream of this engine's previous call when it is another one: the
        staging tensors of ``upload`` and the packed buffers are reused call after call (the library orders its own scratch
        the same way, tsff_set_stream).  Not inside graph capture: the capture contract (tsff.h) keeps one stream."""
        torch = self.torch
        s = torch.cuda.current_stream(self.device)
        last = self._last_stream
        if last is not None and last != s and not torch.cuda.is_current_stream_capturing():
            s.wait_stream(last)
        self._last_stream = s
        return s

    def _sync_stream(self):
        s = self._follow_stream()
        L.check(self.lib, self.h, self.lib.tsff_set_stream(self.h, C.c_void_p(s.cuda_stream)))

    def reserve(self, B: int):
        """tsff_reserve: size the workspace for calls of up to B lineouts now, so that they allocate nothing -- the first step
        of the graph-capture contract of tsff.h (reserve, one eager call with the same mask and slots, synchronise, capture)."""
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_reserve(self.h, int(B)))

    def _vec(self, a, B):
        """amplitude-like input -> [B] device vector."""
        t = self.dev(a).reshape(-1)
        if t.numel() == 1 and B > 1:
            t = t.expand(B).contiguous()
        assert t.numel() == B, f"expected {B} amplitudes, got {t.numel()}"
        return t

    def _mat(self, a, B):
        """noise/data-like input -> [B, 1024] device matrix or None for an all-zero scalar."""
        if a is None:
            return None
        if not isinstance(a, self.torch.Tensor):
            arr = np.asarray(a, dtype=np.float64)
            if arr.size == 1 and float(arr.reshape(-1)[0]) == 0.0:
                return None
            if arr.size != B * L.NBINS:
                arr = np.broadcast_to(arr.reshape(-1, 1) if arr.ndim <= 1 and arr.size in (1, B) else arr, (B, L.NBINS))
            a = arr
        t = self.dev(a)
        return t.reshape(B, L.NBINS).contiguous()

    def _batch_args(self, X, batch, fe=None, need_data=True):
        """The batch arguments of an entry point: -> (tensors, args).  ``args``: the C ABI's ``params, fe, e_data, i_data, e_amps,
        i_amps, noise_e, noise_i, B`` for the lineouts of ``X`` [B, NP] (a feature that is not loaded: null; ``need_data=False``:
        null data); ``tensors``: the device tensors behind them -- hold on to it until the library call has returned."""
        B = X.shape[0]
        ed = self._mat(batch["e_data"], B) if need_data and self.load_ele else None
        idt = self._mat(batch["i_data"], B) if need_data and self.load_ion else None
        ea = self._vec(batch["e_amps"], B) if self.load_ele else None
        ia = self._vec(batch["i_amps"], B) if self.load_ion else None
        ne_, ni_ = self._mat(batch.get("noise_e"), B), self._mat(batch.get("noise_i"), B)
        fe_d = self.dev(fe)
        p = self._ptr
        return (X, fe_d, ed, idt, ea, ia, ne_, ni_), (p(X), p(fe_d), p(ed), p(idt), p(ea), p(ia), p(ne_), p(ni_), B)

    # ---- entry points ---------------------------------------------------------------------------
    def chi_table(self, fe):
        torch = self.torch
        fe_d = self.dev(fe).reshape(-1, self.nvx)
        W = torch.empty((fe_d.shape[0], L.NXI2), dtype=torch.float64, device=self.device)
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_chi_table(self.h, self._ptr(fe_d), fe_d.shape[0], self._ptr(W)))
        return W

    def form_factor(self, feature, phys, fe=None):
        """Raw FormFactor.__call__: phys [B, NP] PHYSICAL parameters -> P [B, G, npts, n_angles]."""
        torch = self.torch
        phys_d = self.dev(phys).reshape(-1, self.NP)
        B = phys_d.shape[0]
        fe_d = self.dev(fe)
        G, NA = int(self._cfg_struct.num_grad_points), int(self._cfg_struct.n_angles)
        P = torch.empty((B, G, self.npts, NA), dtype=torch.float64, device=self.device)
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_form_factor(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), B, self._ptr(P)))
        return P

    def form_factor_grad(self, feature, phys, fe, Pbar, want_fe=False):
        """Adjoint of form_factor: Pbar [B, G, npts, n_angles] -> (grad_phys [B, NP], grad_fe [B, nvx] or None)."""
        torch = self.torch
        phys_d = self.dev(phys).reshape(-1, self.NP)
        B = phys_d.shape[0]
        fe_d, Pb = self.dev(fe), self.dev(Pbar)
        gp = torch.empty((B, self.NP), dtype=torch.float64, device=self.device)
        gf = torch.empty((B, int(self._cfg_struct.nvx)), dtype=torch.float64, device=self.device) if want_fe else None
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_form_factor_grad(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), B,
                                                                 self._ptr(Pb), self._ptr(gp), self._ptr(gf)))
        return gp, gf

    def form_factor_jvp(self, feature, phys, fe, phys_dot, fe_dot=None, want_P=False):
        """Forward mode of form_factor (tsff_form_factor_jvp): phys_dot [n_dir, B, NP] and fe_dot [n_dir, B, nvx] (or None: no
        direction of f_e) -> (P [B, G, npts, n_angles] or None, P_dot [n_dir, B, G, npts, n_angles]) as CUDA tensors,
        P_dot[k] = dP/dphys . phys_dot[k] + dP/dfe . fe_dot[k]; nothing is synchronised."""
        torch = self.torch
        phys_d = self.dev(phys).reshape(-1, self.NP)
        B = phys_d.shape[0]
        pd = self.dev(phys_dot).reshape(-1, B, self.NP)
        n_dir = int(pd.shape[0])
        fe_d = self.dev(fe)
        fd = self.dev(fe_dot)
        if fd is not None:
            fd = fd.reshape(n_dir, B, self.nvx)
        G, NA = int(self._cfg_struct.num_grad_points), int(self._cfg_struct.n_angles)
        P = torch.empty((B, G, self.npts, NA), dtype=torch.float64, device=self.device) if want_P else None
        Pd = torch.empty((n_dir, B, G, self.npts, NA), dtype=torch.float64, device=self.device)
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_form_factor_jvp(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), B, n_dir,
                                                                self._ptr(pd), self._ptr(fd), self._ptr(P), self._ptr(Pd)))
        return P, Pd

    def form_factor_2d(self, feature, phys, fe2d, ud_angle=0.0, va_angle=0.0, point_range=None, out=None, save=False):
        """FormFactor.calc_in_2D: phys [B, NP] PHYSICAL parameters, fe2d [nv, nv] (shared) or [B, nv, nv]
        -> P [B, G, npts, n_angles].  ``point_range = (begin, end)`` evaluates that slice of the flat point list only
        (the rest of ``out`` / a zero-filled result is untouched): the sharding unit of the multi-GPU path."""
        torch = self.torch
        phys_d = self.dev(phys).reshape(-1, self.NP)
        B = phys_d.shape[0]
        fe_d = self.dev(fe2d)
        shared = fe_d.dim() == 2
        nv = int(fe_d.shape[-1])
        assert fe_d.shape[-2] == nv and (shared or fe_d.shape[0] == B)
        G, NA = int(self._cfg_struct.num_grad_points), int(self._cfg_struct.n_angles)
        if out is not None:
            P = out
        else:
            P = (torch.zeros if point_range is not None else torch.empty)((B, G, self.npts, NA), dtype=torch.float64, device=self.device)
        lo, hi = point_range if point_range is not None else (0, -1)
        self._sync_stream()
        if save and shared and nv <= 256:   # keep the projection records for form_factor_2d_grad(use_saved=True)
            token = C.c_uint64(0)
            rc = self.lib.tsff_form_factor_2d_save(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), nv, float(ud_angle),
                                                   float(va_angle), B, int(lo), int(hi), self._ptr(P), C.byref(token))
            # the library ties the records to the buffers they were made from: keep those buffers (and what the caller
            # passed) so that the adjoint can present the very same ones
            keep = lambda a: a if isinstance(a, torch.Tensor) else np.array(a, dtype=np.float64, copy=True)
            self._saved_2d = dict(phys_in=keep(phys), fe_in=keep(fe2d), phys_d=phys_d, fe_d=fe_d, token=int(token.value))
        else:
            self._saved_2d = None
            rc = self.lib.tsff_form_factor_2d_range(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), nv, int(shared),
                                                    float(ud_angle), float(va_angle), B, int(lo), int(hi), self._ptr(P))
        L.check(self.lib, self.h, rc)
        return P

    def form_factor_2d_grad(self, feature, phys, fe2d, Pbar, ud_angle=0.0, va_angle=0.0, want_table=True, point_range=None,
                            use_saved=False, saved_token=None):
        """Adjoint of form_factor_2d (one shared table): Pbar [B, G, npts, n_angles] ->
        (grad_phys [B, NP], grad_fe2d [nv, nv] or None) as device tensors.  ``point_range = (begin, end)``: the
        contributions of that slice of the flat point list only (to be summed over the ranks of a node)."""
        torch = self.torch
        saved = getattr(self, "_saved_2d", None) if use_saved else None
        if saved is not None and self._same_input(phys, saved["phys_in"], saved["phys_d"]) and self._same_input(fe2d, saved["fe_in"], saved["fe_d"]):
            phys_d, fe_d = saved["phys_d"], saved["fe_d"]   # the buffers the projection records were made from
        else:   # other inputs than the saving forward saw (or no records): the adjoint does its own sampling
            saved = None
            phys_d, fe_d = self.dev(phys).reshape(-1, self.NP), self.dev(fe2d)
        B = phys_d.shape[0]
        Pb = self.dev(Pbar)
        assert fe_d.dim() == 2 and fe_d.shape[0] == fe_d.shape[1]
        nv = int(fe_d.shape[0])
        gp = torch.empty((B, self.NP), dtype=torch.float64, device=self.device)
        gf = torch.empty((nv, nv), dtype=torch.float64, device=self.device) if want_table else None
        self._sync_stream()
        lo, hi = point_range if point_range is not None else (0, -1)
        rc = self.lib.tsff_form_factor_2d_grad(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), nv, float(ud_angle),
                                               float(va_angle), B, int(lo), int(hi),
                                               C.c_uint64(int(saved_token) if saved_token is not None else (saved["token"] if saved is not None else 0)),
                                               self._ptr(Pb), self._ptr(gp), self._ptr(gf))
        L.check(self.lib, self.h, rc)
        return gp, gf

    def form_factor_2d_jvp(self, feature, phys, fe2d, phys_dot, fe2d_dot=None, ud_angle=0.0, va_angle=0.0, want_P=False, point_range=None):
        """Forward mode of form_factor_2d for one shared table, nv <= 256 (tsff_form_factor_2d_jvp): phys_dot [n_dir, B, NP] and
        fe2d_dot [n_dir, nv, nv] (or None: no table direction) -> (P [B, G, npts, n_angles] or None, P_dot [n_dir, B, G, npts,
        n_angles]) as CUDA tensors, P_dot[k] = dP/dphys . phys_dot[k] + dP/dfe2d . fe2d_dot[k]; nothing is synchronised.
        ``point_range = (begin, end)``: that slice of the flat point list only, the rest zero.  The call runs a saving forward of its
        own: the records of an earlier ``form_factor_2d(save=True)`` are gone after it."""
        torch = self.torch
        phys_d = self.dev(phys).reshape(-1, self.NP)
        B = phys_d.shape[0]
        fe_d = self.dev(fe2d)
        assert fe_d.dim() == 2 and fe_d.shape[0] == fe_d.shape[1], "form_factor_2d_jvp takes one shared table"
        nv = int(fe_d.shape[0])
        pd = self.dev(phys_dot).reshape(-1, B, self.NP)
        n_dir = int(pd.shape[0])
        fd = self.dev(fe2d_dot)
        if fd is not None:
            fd = fd.reshape(n_dir, nv, nv)
        G, NA = int(self._cfg_struct.num_grad_points), int(self._cfg_struct.n_angles)
        new = torch.zeros if point_range is not None else torch.empty
        P = new((B, G, self.npts, NA), dtype=torch.float64, device=self.device) if want_P else None
        Pd = new((n_dir, B, G, self.npts, NA), dtype=torch.float64, device=self.device)
        lo, hi = point_range if point_range is not None else (0, -1)
        self._sync_stream()
        self._saved_2d = None
        rc = self.lib.tsff_form_factor_2d_jvp(self.h, int(feature), self._ptr(phys_d), self._ptr(fe_d), nv, float(ud_angle), float(va_angle),
                                              B, n_dir, self._ptr(pd), self._ptr(fd), int(lo), int(hi), self._ptr(P), self._ptr(Pd))
        L.check(self.lib, self.h, rc)
        return P, Pd

    def _same_input(self, a, ref, ref_dev) -> bool:
        """Is ``a`` what the saving forward was given?  A host array equal to the copy kept at the save, or a device tensor on
        the same memory (a device tensor rewritten in place between the two calls cannot be told apart: do not do that)."""
        torch = self.torch
        if isinstance(a, torch.Tensor):
            return a is ref or (a.is_cuda and a.data_ptr() == ref_dev.data_ptr() and a.numel() == ref_dev.numel())
        if isinstance(ref, torch.Tensor):
            return False
        a = np.asarray(a)
        return a.size == ref.size and bool(np.array_equal(a.reshape(ref.shape), ref))

    def ats_setup(self, weights, ang_axis, stddev_lam, stddev_ang, lam_step=1, ang_step=1, row_start=0, row_end=None,
                  irf_cutoff_sigmas=12.0):
        """Static configuration of the angular (ARTS) instrument chain: weight matrix [n_px, n_angles], the calibrated
        angle axis sas["angAxis"] [n_px] and the two Gaussian widths (FWHM / 2.3548, irf.py:23-24)."""
        W = np.ascontiguousarray(weights, dtype=np.float64)
        n_px = W.shape[0]
        assert W.shape[1] == int(self._cfg_struct.n_angles)
        lamE = wavelength_axis_nm(self.cfg["other"]["lamrangE"], self.npts)
        ta, da = gaussian_taps(np.asarray(ang_axis, dtype=np.float64), float(stddev_ang), irf_cutoff_sigmas)
        ta, offa = binned_taps(ta, da, 1)
        tl, dl = gaussian_taps(lamE, float(stddev_lam), irf_cutoff_sigmas)
        tl, offl = binned_taps(tl, dl, 1)
        c = L.TsffAtsConfig()
        c.n_px = n_px
        keep = []
        a, c.weights = _as_c(W, np.float64); keep.append(a)
        a, c.taps_ang = _as_c(ta, np.float64); keep.append(a)
        a, c.taps_lam = _as_c(tl, np.float64); keep.append(a)
        a, c.lam_axis = _as_c(lamE, np.float64); keep.append(a)
        c.n_taps_ang, c.tap_off_ang, c.n_taps_lam, c.tap_off_lam = ta.size, offa, tl.size, offl
        c.lam_step, c.ang_step = int(lam_step), int(ang_step)
        c.row_start = int(row_start)
        c.row_end = int(row_end if row_end is not None else n_px // ang_step)
        L.check(self.lib, self.h, self.lib.tsff_ats_setup(self.h, C.byref(c)))
        self._ats_shape = (c.row_end - c.row_start, self.npts // int(lam_step))

    def ats_spectrum(self, P, e_amps, lam, amp1, amp2):
        """P [G, npts, n_angles] (one image) -> ThryE [rows, npts / lam_step]."""
        torch = self.torch
        Pd = self.dev(P)
        ea = self.dev(np.broadcast_to(np.asarray(e_amps, dtype=np.float64).reshape(-1), (self._ats_shape[0],)).copy()
                      if not torch.is_tensor(e_amps) else e_amps.reshape(-1))
        assert ea.numel() == self._ats_shape[0]
        out = torch.empty(self._ats_shape, dtype=torch.float64, device=self.device)
        self._sync_stream()
        rc = self.lib.tsff_ats_spectrum(self.h, self._ptr(Pd), self._ptr(ea), float(lam), float(amp1), float(amp2), self._ptr(out))
        L.check(self.lib, self.h, rc)
        return out

    def ats_adjoint(self, P, e_amps, lam, amp1, amp2, Ebar):
        """Reverse of ats_spectrum: Ebar [rows, n_lam] -> (Pbar [G, npts, n_angles] device tensor, (amp1_bar, amp2_bar))."""
        torch = self.torch
        Pd, Eb = self.dev(P), self.dev(Ebar)
        ea = self.dev(np.broadcast_to(np.asarray(e_amps, dtype=np.float64).reshape(-1), (self._ats_shape[0],)).copy()
                      if not torch.is_tensor(e_amps) else e_amps.reshape(-1))
        assert tuple(Eb.shape) == tuple(self._ats_shape)
        Pbar = torch.empty_like(Pd)
        ab = (C.c_double * 2)()
        self._sync_stream()
        rc = self.lib.tsff_ats_adjoint(self.h, self._ptr(Pd), self._ptr(ea), float(lam), float(amp1), float(amp2), self._ptr(Eb),
                                       self._ptr(Pbar), ab)
        L.check(self.lib, self.h, rc)
        return Pbar, (float(ab[0]), float(ab[1]))

    def ats_jvp(self, P, P_dot, e_amps, lam, amp1, amp2, amp_dot=None, want_E=False):
        """Forward mode of ats_spectrum (tsff_ats_jvp): P [G, npts, n_angles], P_dot [n_dir, G, npts, n_angles], amp_dot
        [n_dir, 2] the tangents of (amp1, amp2) (None: zeros) -> (ThryE [rows, n_lam] or None, ThryE_dot [n_dir, rows, n_lam])
        as CUDA tensors; nothing is synchronised."""
        torch = self.torch
        Pd = self.dev(P)
        Pt = self.dev(P_dot).reshape((-1,) + tuple(Pd.shape))
        n_dir = int(Pt.shape[0])
        ea = self.dev(np.broadcast_to(np.asarray(e_amps, dtype=np.float64).reshape(-1), (self._ats_shape[0],)).copy()
                      if not torch.is_tensor(e_amps) else e_amps.reshape(-1))
        assert ea.numel() == self._ats_shape[0]
        ad = np.zeros((n_dir, 2)) if amp_dot is None else np.ascontiguousarray(amp_dot, dtype=np.float64).reshape(n_dir, 2)
        E = torch.empty(self._ats_shape, dtype=torch.float64, device=self.device) if want_E else None
        Ed = torch.empty((n_dir,) + tuple(self._ats_shape), dtype=torch.float64, device=self.device)
        self._sync_stream()
        rc = self.lib.tsff_ats_jvp(self.h, self._ptr(Pd), self._ptr(Pt), n_dir, self._ptr(ea), float(lam), float(amp1), float(amp2),
                                   ad.ctypes.data_as(L.c_double_p), self._ptr(E), self._ptr(Ed))
        L.check(self.lib, self.h, rc)
        return E, Ed

    def forward(self, params, e_amps, i_amps, noise_e=None, noise_i=None, fe=None):
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        keep, ba = self._batch_args(X, dict(e_amps=e_amps, i_amps=i_amps, noise_e=noise_e, noise_i=noise_i), fe, need_data=False)
        # (the kernel writes every entry of a loaded feature; a feature that is not loaded comes back as zeros)
        E = (torch.empty if self.load_ele else torch.zeros)((B, L.NBINS), dtype=torch.float64, device=self.device)
        I = (torch.empty if self.load_ion else torch.zeros)((B, L.NBINS), dtype=torch.float64, device=self.device)
        self._sync_stream()
        rc = self.lib.tsff_forward(self.h, *ba[:2], *ba[4:], self._ptr(E), self._ptr(I))   # (no data arguments)
        L.check(self.lib, self.h, rc)
        return E, I

    def loss_weights(self, B_global, i_norm, e_norm, ion_loss_scale=1.0):
        """The factor each masked sum carries in the total loss (loss_function.py:190-267, 335-338)
        for a nanmean over B_global x 1024 entries and constant denominators i_norm^2 / e_norm^2."""
        c = 0.5 if (self.fit_blue and self.fit_red) else 1.0
        w = np.zeros(3)
        if self.fit_iaw and self.n_iaw:
            w[0] = ion_loss_scale / (B_global * self.n_iaw * i_norm**2)
        if self.fit_blue and self.n_blue:
            w[1] = c / (B_global * self.n_blue * e_norm**2)
        if self.fit_red and self.n_red:
            # the reference halves (blue + red) only when blue is fitted too (:262-264)
            w[2] = c / (B_global * self.n_red * e_norm**2)
        if self.cfg.get("optimizer", {}).get("loss_method", "l2") in ("log-cosh", "poisson"):
            # these functionals ignore the denominator (loss_function.py:414-417)
            w[0] *= i_norm**2
            w[1] *= e_norm**2
            w[2] *= e_norm**2
        return w

    def loss_grad(self, params, batch, weights, grad_mask, fe=None, want_spectra=False, out=None, want_fe_grad=False):
        """-> (loss_terms[3], grad[B, NP], ThryE, ThryI) as CUDA tensors; nothing is synchronised.
        ``want_fe_grad`` (fe_mode PER_LINEOUT): a fifth result, d loss / d fe [B, nvx]."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        keep, ba = self._batch_args(X, batch, fe)
        if out is None:
            terms = torch.empty(3, dtype=torch.float64, device=self.device)
            grad = torch.empty((B, self.NP), dtype=torch.float64, device=self.device)
        else:
            terms, grad = out
        E = torch.zeros((B, L.NBINS), dtype=torch.float64, device=self.device) if want_spectra else None
        I = torch.zeros((B, L.NBINS), dtype=torch.float64, device=self.device) if want_spectra else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        gm = np.ascontiguousarray(grad_mask, dtype=np.uint8)
        self._sync_stream()
        if want_fe_grad:
            gfe = torch.empty((B, self.nvx), dtype=torch.float64, device=self.device)
            rc = self.lib.tsff_loss_grad_fe(self.h, *ba, w.ctypes.data_as(L.c_double_p), gm.ctypes.data_as(L.c_uint8_p),
                                            self._ptr(terms), self._ptr(grad), self._ptr(gfe), self._ptr(E), self._ptr(I))
            L.check(self.lib, self.h, rc)
            return terms, grad, E, I, gfe
        rc = self.lib.tsff_loss_grad(self.h, *ba, w.ctypes.data_as(L.c_double_p), gm.ctypes.data_as(L.c_uint8_p),
                                     self._ptr(terms), self._ptr(grad), self._ptr(E), self._ptr(I))
        L.check(self.lib, self.h, rc)
        return terms, grad, E, I

    def loss_hess(self, params, batch, weights, active_slots, fe=None):
        """Exact per-lineout Hessian of ``_loss_for_hess_fn_`` (denominators |data| + 1e-10 for l1 / l2, sum reduce) w.r.t. the
        normalised leaves of ``active_slots`` (ravel order): -> (loss_terms[3], grad[B, P], hess[B, P, P]) as CUDA tensors of
        sum_k weights[k] S_k; nothing is synchronised (tsff_loss_hess)."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, batch, fe)
        terms = torch.empty(3, dtype=torch.float64, device=self.device)
        grad = torch.empty((B, P), dtype=torch.float64, device=self.device)
        hess = torch.empty((B, P, P), dtype=torch.float64, device=self.device)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._sync_stream()
        rc = self.lib.tsff_loss_hess(self.h, *ba, w.ctypes.data_as(L.c_double_p), act.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                     self._ptr(terms), self._ptr(grad), self._ptr(hess))
        L.check(self.lib, self.h, rc)
        return terms, grad, hess

    def angular_loss_hess(self, leaves, active_slots, e_data, noise_e, e_amps, wcol, method, fe=None, want_images=False):
        """Exact Hessian of ``_loss_for_hess_fn_`` on an angular (ARTS) deck with a 1-D f_e (tsff_angular_loss_hess; ``ats_setup`` has
        run): ``leaves`` [NP] the normalised row of the one plasma condition, ``active_slots`` in ravel order (the DLM order among
        them on an FE_DLM engine), ``e_data`` / ``noise_e`` [rows, n_lam] (noise_e None: zero), ``e_amps`` [rows], ``wcol`` [n_lam] the
        weight of every column, ``method`` the loss functional's name, ``fe`` [nvx] on an FE_PER_LINEOUT engine.  -> a dict of CUDA
        tensors: ``loss`` [1], ``grad`` [n], ``hess`` [n, n] (symmetric), ``gn`` [n, n] (its Gauss-Newton part); with ``want_images``
        also ``E`` [rows, n_lam], ``E1`` [n, rows, n_lam], ``E2`` [n (n + 1) / 2, rows, n_lam] (pairs a <= c, row-major over the upper
        triangle) and ``phys`` [NP].  Nothing is synchronised."""
        torch = self.torch
        rows, nJ = self._ats_shape
        x = self.dev(leaves).reshape(-1)
        assert x.numel() == self.NP, f"expected {self.NP} leaves, got {x.numel()}"
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        n = int(act.size)
        d = self.dev(e_data).reshape(rows, nJ)
        nz = None if noise_e is None else self.dev(noise_e)
        if nz is not None and nz.numel() != rows * nJ:
            nz = nz.expand(rows, nJ).contiguous()
        ea = self.dev(np.broadcast_to(np.asarray(e_amps, dtype=np.float64).reshape(-1), (rows,)).copy()
                      if not torch.is_tensor(e_amps) else e_amps.reshape(-1))
        assert ea.numel() == rows
        wc = self.dev(wcol).reshape(-1)
        assert wc.numel() == nJ
        fe_d = self.dev(fe)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
        out = dict(loss=new(1), grad=new(n), hess=new(n, n), gn=new(n, n))
        if want_images:
            out.update(E=new(rows, nJ), E1=new(n, rows, nJ), E2=new(n * (n + 1) // 2, rows, nJ), phys=new(self.NP))
        p = self._ptr
        self._sync_stream()
        rc = self.lib.tsff_angular_loss_hess(self.h, p(x), p(fe_d), act.ctypes.data_as(C.POINTER(C.c_int32)), n, p(d), p(nz), p(ea), p(wc),
                                             int(L.LOSS_METHODS[method]), p(out["loss"]), p(out["grad"]), p(out["hess"]), p(out["gn"]),
                                             p(out.get("E")), p(out.get("E1")), p(out.get("E2")), p(out.get("phys")))
        L.check(self.lib, self.h, rc)
        return out

    def spectrum_jacobian(self, params, e_amps, i_amps, active_slots, fe=None):
        """Jacobian of the model spectra (``forward`` without the noise) w.r.t. the normalised leaves of ``active_slots`` (ravel
        order): -> (JE, JI), CUDA tensors [B, P, 1024]; a feature that is not loaded returns ``None``.  Nothing is synchronised
        (tsff_spectrum_jacobian: the table convention of ``loss_hess``).  ``last_launch()`` names the form that ran,
        ``k_jac_sweep<n_ion, W, rows>``: the row form (1-2 ion species, one gradient point, no DLM order among the leaves) costs
        about two forwards whatever P; the tangent form carries W = 3 leaves per sweep; W = 1 -- a spectrum too long for the LDS
        with three tangents, e.g. 5 points per pixel -- runs one full sweep per leaf, no faster than central differences."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, dict(e_amps=e_amps, i_amps=i_amps), fe, need_data=False)
        JE = torch.empty((B, P, L.NBINS), dtype=torch.float64, device=self.device) if self.load_ele else None
        JI = torch.empty((B, P, L.NBINS), dtype=torch.float64, device=self.device) if self.load_ion else None
        self._sync_stream()
        rc = self.lib.tsff_spectrum_jacobian(self.h, *ba[:2], *ba[4:6], B, act.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                             self._ptr(JE), self._ptr(JI))
        L.check(self.lib, self.h, rc)
        return JE, JI

    def loss_gauss_newton(self, params, batch, weights, active_slots, fe=None):
        """Gauss-Newton curvature of the loss of ``loss_hess``: -> (loss_terms[3], grad[B, P], gn[B, P, P]) as CUDA tensors,
        gn[b] = sum_k weights[k] sum_{j in mask_k} l''(d_j, t_j) J[:, j] J[:, j]^T (symmetric, positive semi-definite), grad
        that of ``loss_hess``; nothing is synchronised (tsff_loss_gauss_newton; the Jacobian is not written to memory)."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, batch, fe)
        terms = torch.empty(3, dtype=torch.float64, device=self.device)
        grad = torch.empty((B, P), dtype=torch.float64, device=self.device)
        gn = torch.empty((B, P, P), dtype=torch.float64, device=self.device)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._sync_stream()
        rc = self.lib.tsff_loss_gauss_newton(self.h, *ba, w.ctypes.data_as(L.c_double_p), act.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                             self._ptr(terms), self._ptr(grad), self._ptr(gn))
        L.check(self.lib, self.h, rc)
        return terms, grad, gn

    def pack_fe_rows(self, terms, grad, gfe, active_slots, B_global=None, b_offset=0, out=None):
        """The packed buffer ``[3 | (P + nvx) x B_global]`` of a free-form f_e step from the outputs of ``loss_grad(want_fe_grad=True)``
        (tsff_pack_fe_rows: one transposing kernel, this rank's columns filled, the others zero)."""
        torch = self.torch
        B = int(grad.shape[0])
        Bg = B if B_global is None else int(B_global)
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        n = 3 + (act.size + self.nvx) * Bg
        packed = out if out is not None else torch.empty(n, dtype=torch.float64, device=self.device)
        assert packed.numel() == n
        self._sync_stream()
        L.check(self.lib, self.h, self.lib.tsff_pack_fe_rows(self.h, self._ptr(terms), self._ptr(grad), self._ptr(gfe), B,
                                                             act.ctypes.data_as(C.POINTER(C.c_int32)), int(act.size), Bg, int(b_offset),
                                                             self._ptr(packed)))
        return packed

    def loss_grad_packed(self, params, batch, weights, grad_mask, active_slots, B_global=None, b_offset=0, want_spectra=False, out=None):
        """tsff_loss_grad_packed: -> (packed [3 + P * B_global] CUDA tensor, ThryE, ThryI).  packed = [S_iaw, S_blue, S_red |
        gradient, trainable leaves outermost, lineouts of the GLOBAL batch innermost]; this rank's B lineouts fill the
        columns [b_offset, b_offset + B), every other column is written as zero -- the buffer of the step's one in-place
        all-reduce and of the single device-to-host copy.  The buffer is persistent per (P, B_global)."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        Bg = int(B_global) if B_global is not None else B
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        keep, ba = self._batch_args(X, batch)   # (a null fe)
        if out is None:
            key = ("packed", act.size, Bg)
            out = self._staging.get(key)
            if out is None:
                out = torch.zeros(3 + act.size * Bg, dtype=torch.float64, device=self.device)
                self._staging[key] = out
        assert out.numel() == 3 + act.size * Bg and out.is_contiguous()
        E = torch.zeros((B, L.NBINS), dtype=torch.float64, device=self.device) if want_spectra else None
        I = torch.zeros((B, L.NBINS), dtype=torch.float64, device=self.device) if want_spectra else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        gm = np.ascontiguousarray(grad_mask, dtype=np.uint8)
        self._sync_stream()
        rc = self.lib.tsff_loss_grad_packed(self.h, *ba, w.ctypes.data_as(L.c_double_p), gm.ctypes.data_as(L.c_uint8_p),
                                            act.ctypes.data_as(C.POINTER(C.c_int32)), int(act.size), Bg, int(b_offset), self._ptr(out),
                                            self._ptr(E), self._ptr(I))
        L.check(self.lib, self.h, rc)
        return out, E, I

    def adam_fit(self, params, batch, weights, active_slots, n_steps, hyper, state=None, best=None, step0=0, loss_hist=True,
                 fe=None):
        """tsff_adam_fit: ``n_steps`` Adam steps of the active leaves on the device, enqueued at once; nothing is synchronised.
        -> (params [B, NP], state [2, P, B] (mu, nu), loss_hist [n_steps] or None, best [1 + B * NP] = [best loss | best params])
        as CUDA tensors.  ``params``, ``state`` and ``best`` are updated in place when they are float64 CUDA tensors already
        (pass the returned ones to the next chunk, with ``step0`` the steps done so far); otherwise they are copied to new
        ones.  ``state=None`` starts a fit (zeros), ``best=None`` starts the best tracking at [1e16 | params].
        ``hyper`` = (lr, b1, b2, eps).  ``fe`` (fe_mode PER_LINEOUT): the tabulated f_e, a constant of the fit."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, batch, fe)
        state = torch.zeros((2, P, B), dtype=torch.float64, device=self.device) if state is None else self.dev(state)
        assert state.numel() == 2 * P * B, f"state must hold 2 x {P} x {B} values"
        if best is None:
            best = torch.cat([torch.full((1,), 1e16, dtype=torch.float64, device=self.device), X.reshape(-1)])
        else:
            best = self.dev(best)
        assert best.numel() == 1 + B * self.NP, f"best must hold 1 + {B} x {self.NP} values"
        hist = torch.empty(max(int(n_steps), 0), dtype=torch.float64, device=self.device) if loss_hist else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        hy = np.ascontiguousarray(hyper, dtype=np.float64)
        assert hy.size == 4, "hyper = (lr, b1, b2, eps)"
        self._sync_stream()
        rc = self.lib.tsff_adam_fit(self.h, *ba, w.ctypes.data_as(L.c_double_p),
                                    act.ctypes.data_as(C.POINTER(C.c_int32)), P, int(n_steps), int(step0),
                                    hy.ctypes.data_as(L.c_double_p), self._ptr(state), self._ptr(hist), self._ptr(best))
        L.check(self.lib, self.h, rc)
        return X, state, hist, best

    def angular_fit(self, leaves, spec: dict, data: dict, n_epochs, state=None, epoch0=0, loss_hist=True, best_hist=False):
        """tsff_angular_fit: ``n_epochs`` epochs of the angular (ARTS) fit on the device, enqueued at once; nothing is synchronised
        (call ats_setup first).  ``spec``: the fields of tsff_angular_spec (generator, nv, active_slots, loss_method, un, dvx,
        method, lr, b1, b2, eps, decay; 2-D generators: ud_angle, va_angle).  ``data``: device tensors gen_data, e_data and
        noise_e [rows, nJ], wcol [nJ], e_amps [rows].  ``leaves``: the NP normalised leaves, then the generator's tail:
          generator    tail                      data["gen_data"]                      spec also carries          best_hist row
          ANG_TABLE2D  none                      the table [nv, nv]                                               NP
          ANG_DLM      none                      distribution.dlm_table(nv) | M_AXIS                              NP
          ANG_ARB2V    fval2d [nv^2]             None                                  learn_log                  NP
          ANG_SPH      sph.get_params() [n_gen]  distribution.sph_gen_data(sph)[0]     its meta, sph_gen_data[1]  NP + n_gen
          ANG_ARB1V    fval [nv]                 distribution.arb1v_gen_data(nv)                                  NP + nv
        -> (leaves, state = (moments, best, ctl), loss_hist [n_epochs] or None, best_hist (NaN rows: no best yet) or None) as CUDA
        tensors.  ``leaves`` and ``state`` are updated in place when they are CUDA tensors already (pass the returned ones to the next
        chunk, with ``epoch0`` the epochs done so far).  ``state=None``: zero moments, best = [100 | leaves] (angular_optax), ctl zeros."""
        torch = self.torch
        x = self.dev(leaves).reshape(-1)
        act = np.ascontiguousarray(spec.get("active_slots", ()), dtype=np.int32)
        n = int(act.size) + int(x.numel()) - self.NP
        adam = spec["method"] == L.ANG_ADAM
        if state is None:
            best = torch.cat([torch.full((1,), 100.0, dtype=torch.float64, device=self.device), x])
            state = (torch.zeros((2 if adam else 1) * n, dtype=torch.float64, device=self.device), best,
                     torch.zeros(8, dtype=torch.int32, device=self.device))
        mom, best, ctl = state
        assert mom.numel() == (2 if adam else 1) * n and best.numel() == 1 + x.numel() and ctl.dtype == torch.int32
        hist = torch.empty(max(int(n_epochs), 0), dtype=torch.float64, device=self.device) if loss_hist else None
        n_hist = int(x.numel()) if int(spec["generator"]) in L.ANG_HIST_TAIL else self.NP
        bh = torch.full((max(int(n_epochs), 0), n_hist), float("nan"), dtype=torch.float64, device=self.device) if best_hist else None
        c = L.TsffAngularSpec()
        c.generator, c.nv, c.learn_log = int(spec["generator"]), int(spec["nv"]), int(bool(spec.get("learn_log", False)))
        c.n_active, c.active_slots = int(act.size), act.ctypes.data_as(C.POINTER(C.c_int32))
        c.loss_method, c.un = int(spec["loss_method"]), float(spec["un"])
        c.ud_angle, c.va_angle, c.dvx = float(spec.get("ud_angle", 0.0)), float(spec.get("va_angle", 0.0)), float(spec["dvx"])
        c.method = int(spec["method"])
        c.lr, c.b1, c.b2, c.eps, c.decay = (float(spec.get(k, 0.0)) for k in ("lr", "b1", "b2", "eps", "decay"))
        c.n_epochs, c.epoch0 = int(n_epochs), int(epoch0)
        c.sph_type, c.n_harm, c.nvr, c.n_gen = (int(spec.get(k, 0)) for k in ("sph_type", "n_harm", "nvr", "n_gen"))
        self._sync_stream()
        rc = self.lib.tsff_angular_fit(self.h, C.byref(c), self._ptr(x), self._ptr(data.get("gen_data")), self._ptr(data["e_data"]),
                                       self._ptr(data["noise_e"]), self._ptr(data["wcol"]), self._ptr(data["e_amps"]), self._ptr(mom),
                                       self._ptr(best), self._ptr(ctl), self._ptr(hist), self._ptr(bh))
        L.check(self.lib, self.h, rc)
        return x, (mom, best, ctl), hist, bh

    def _sph_args(self, meta: dict, dvx):
        return [int(meta[k]) for k in ("sph_type", "n_harm", "nv", "nvr", "n_gen")] + [float(dvx)]

    def sph_table(self, theta, gen_data, meta: dict, dvx=None, out=None):
        """tsff_sph_table: the SphericalHarmonics generator on the device, ``theta`` [n_gen] (``get_params()`` order) ->
        f_e [nv, nv] (CUDA tensor; nothing is synchronised).  ``gen_data``, ``meta``: distribution.sph_gen_data(sph);
        ``dvx``: vx[1] - vx[0] (default: the reference's grid, 12 / nv)."""
        torch = self.torch
        nv = int(meta["nv"])
        th, gd = self.dev(theta).reshape(-1), self.dev(gen_data)
        assert th.numel() == int(meta["n_gen"]) and gd.numel() == D.sph_gen_layout(meta["sph_type"], meta["n_harm"], nv, meta["nvr"])["size"]
        fe = out if out is not None else torch.empty((nv, nv), dtype=torch.float64, device=self.device)
        self._sync_stream()
        rc = self.lib.tsff_sph_table(self.h, *self._sph_args(meta, 12.0 / nv if dvx is None else dvx), self._ptr(th), self._ptr(gd),
                                     self._ptr(fe))
        L.check(self.lib, self.h, rc)
        return fe

    def sph_table_vjp(self, theta, gen_data, meta: dict, fe_bar, dvx=None, out=None):
        """tsff_sph_table_vjp: ``fe_bar`` [nv, nv] = d loss / d f_e -> d loss / d theta [n_gen] (CUDA tensor; nothing is
        synchronised), exact and bit-reproducible from run to run.  Arguments as :meth:`sph_table`."""
        torch = self.torch
        nv = int(meta["nv"])
        th, gd, fb = self.dev(theta).reshape(-1), self.dev(gen_data), self.dev(fe_bar).reshape(-1)
        assert th.numel() == int(meta["n_gen"]) and fb.numel() == nv * nv
        assert gd.numel() == D.sph_gen_layout(meta["sph_type"], meta["n_harm"], nv, meta["nvr"])["size"]
        g = out if out is not None else torch.empty(int(meta["n_gen"]), dtype=torch.float64, device=self.device)
        self._sync_stream()
        rc = self.lib.tsff_sph_table_vjp(self.h, *self._sph_args(meta, 12.0 / nv if dvx is None else dvx), self._ptr(th),
                                         self._ptr(gd), self._ptr(fb), self._ptr(g))
        L.check(self.lib, self.h, rc)
        return g

    def arb1v_table(self, fval, gen_data, dvx=None, out=None):
        """tsff_arb1v_table: the free-form 1-D generator (Arbitrary1V, distribution.arbitrary_1v) on the device, ``fval`` [nv] ->
        f_e [nv] (CUDA tensor; nothing is synchronised).  ``gen_data``: distribution.arb1v_gen_data(nv); ``dvx``: vx[1] - vx[0]
        (default: the reference's grid, 12 / nv)."""
        torch = self.torch
        fv, gd = self.dev(fval).reshape(-1), self.dev(gen_data).reshape(-1)
        nv = int(fv.numel())
        assert gd.numel() == 2 * nv * nv, "gen_data: S | S^T of the size of fval"
        fe = out if out is not None else torch.empty(nv, dtype=torch.float64, device=self.device)
        assert fe.numel() == nv
        self._sync_stream()
        rc = self.lib.tsff_arb1v_table(self.h, nv, float(12.0 / nv if dvx is None else dvx), self._ptr(fv), self._ptr(gd), self._ptr(fe))
        L.check(self.lib, self.h, rc)
        return fe

    def arb1v_table_vjp(self, fval, gen_data, fe_bar, dvx=None, out=None):
        """tsff_arb1v_table_vjp: ``fe_bar`` [nv] = d loss / d f_e -> d loss / d fval [nv] (CUDA tensor; nothing is synchronised),
        the chain of distribution.arbitrary_1v_vjp, bit-reproducible from run to run.  Arguments as :meth:`arb1v_table`."""
        torch = self.torch
        fv, gd, fb = self.dev(fval).reshape(-1), self.dev(gen_data).reshape(-1), self.dev(fe_bar).reshape(-1)
        nv = int(fv.numel())
        assert gd.numel() == 2 * nv * nv and fb.numel() == nv
        g = out if out is not None else torch.empty(nv, dtype=torch.float64, device=self.device)
        assert g.numel() == nv
        self._sync_stream()
        rc = self.lib.tsff_arb1v_table_vjp(self.h, nv, float(12.0 / nv if dvx is None else dvx), self._ptr(fv), self._ptr(gd),
                                           self._ptr(fb), self._ptr(g))
        L.check(self.lib, self.h, rc)
        return g

    def lbfgs_fit(self, params, batch, weights, active_slots, n_evals, opts=(10, 2.220446049250313e-09, 1e-5, 15000, 15000, 20),
                  state=None, f_hist=True, info=None, fe=None):
        """tsff_lbfgs_fit: ``n_evals`` evaluations of unbounded L-BFGS-B on the active leaves, enqueued at once; nothing is
        synchronised.  -> (params [B, NP], state, f_hist [n_evals] or None, info int32 [4]) as CUDA tensors.  ``params``,
        ``state`` and ``info`` are updated in place when they are CUDA tensors of the right type already (pass the returned
        ones to the next chunk); otherwise they are copied to new ones.  ``state=None`` starts a fit (zeros) at ``params``.
        ``opts`` = (maxcor, ftol, gtol, maxiter, maxfun, maxls).  ``fe`` (fe_mode PER_LINEOUT): a constant of the fit.
        Read the outcome with :meth:`lbfgs_info`."""
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, batch, fe)
        op = np.ascontiguousarray(opts, dtype=np.float64)
        assert op.size == 6, "opts = (maxcor, ftol, gtol, maxiter, maxfun, maxls)"
        if state is None:
            need = C.c_int64(0)
            if self.lib.tsff_lbfgs_state_size(B, P, int(op[0]), C.byref(need)) != 0:
                raise L.TsffError(f"libtsff: no L-BFGS state for B = {B}, {P} leaves, maxcor = {op[0]}")
            state = torch.zeros(need.value, dtype=torch.float64, device=self.device)
        else:
            state = self.dev(state)
        if info is None or not (torch.is_tensor(info) and info.dtype == torch.int32 and info.is_cuda and info.numel() == 4):
            info = torch.zeros(4, dtype=torch.int32, device=self.device)
        hist = torch.empty(max(int(n_evals), 0), dtype=torch.float64, device=self.device) if f_hist else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._sync_stream()
        rc = self.lib.tsff_lbfgs_fit(self.h, *ba, w.ctypes.data_as(L.c_double_p),
                                     act.ctypes.data_as(C.POINTER(C.c_int32)), P, int(n_evals), op.ctypes.data_as(L.c_double_p),
                                     self._ptr(state), int(state.numel()), self._ptr(hist), self._ptr(info))
        L.check(self.lib, self.h, rc)
        return X, state, hist, info

    def lbfgs_info(self, info, state=None) -> dict:
        """The outcome of :meth:`lbfgs_fit` (one synchronising copy, info and the loss together): status (tsadar_amd.lbfgs: RUNNING .. ABNORMAL), scipy's
        termination class ``scipy_status`` (None while running), nit, nfev, nskip, and with ``state`` the loss ``f`` of the last
        accepted iterate."""
        from . import lbfgs

        torch = self.torch
        dv = info.to(torch.float64)   # (exact for int32) -- one copy of the counts and the loss
        if state is not None:
            dv = torch.cat([dv, state[lbfgs.HDR_F0:lbfgs.HDR_F0 + 1]])
        host = self.download(dv)
        v = [int(a) for a in host[:4]]
        out = dict(status=v[0], scipy_status=lbfgs.SCIPY_STATUS.get(v[0]), nit=v[1], nfev=v[2], nskip=v[3])
        if state is not None:
            out["f"] = float(host[4])
        return out

    def lm_fit(self, params, batch, weights, active_slots, n_evals, opts, state=None, hist=False, fe=None):
        """tsff_lm_fit: ``n_evals`` evaluations of the per-lineout Levenberg-Marquardt fit (tsadar_amd.lm) on the active leaves,
        enqueued at once; nothing is synchronised.  -> (params [B, NP], state, x_hist [n_evals, B, P] or None, eval_hist
        [n_evals, B, 1 + P + P * P] (F | G | H) or None) as CUDA tensors.  ``params`` and ``state`` are updated in place when
        they are float64 CUDA tensors already (pass the returned ones to the next chunk); otherwise they are copied to new ones.
        ``state=None`` starts a fit (zeros) at ``params``.  ``opts`` = lm.Options (tau, gtol, ftol, xtol, maxiter, maxfun,
        lam_max).  ``weights``: with ``loss_weights(1, ...)`` every lineout's loss is its own mean loss.  ``fe`` (fe_mode
        PER_LINEOUT): a constant of the fit.  Read the outcome with :meth:`lm_info`."""
        from . import lm

        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        act = np.ascontiguousarray(active_slots, dtype=np.int32)
        P = int(act.size)
        keep, ba = self._batch_args(X, batch, fe)
        op = np.ascontiguousarray(opts, dtype=np.float64)
        assert op.size == 7, "opts = (tau, gtol, ftol, xtol, maxiter, maxfun, lam_max)"
        state = torch.zeros(lm.state_size(B, P), dtype=torch.float64, device=self.device) if state is None else self.dev(state)
        k = max(int(n_evals), 0)
        xh = torch.empty((k, B, P), dtype=torch.float64, device=self.device) if hist else None
        eh = torch.empty((k, B, 1 + P + P * P), dtype=torch.float64, device=self.device) if hist else None
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._sync_stream()
        rc = self.lib.tsff_lm_fit(self.h, *ba, w.ctypes.data_as(L.c_double_p), act.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                  int(n_evals), op.ctypes.data_as(L.c_double_p), self._ptr(state), int(state.numel()),
                                  self._ptr(xh), self._ptr(eh))
        L.check(self.lib, self.h, rc)
        self._lm_shape = (B, P)
        return X, state, xh, eh

    def lm_info(self, state, shape=None) -> dict:
        """The outcome of :meth:`lm_fit` per lineout (one synchronising copy of the state): x [B, P] (the accepted points), f,
        lam, status (tsadar_amd.lm: RUNNING .. BAD_START), nit, nfev.  ``shape`` = (B, P): of the most recent lm_fit by default."""
        from . import lm

        B, P = shape if shape is not None else self._lm_shape
        st = lm.unpack(self.download(state), B, P)
        return dict(x=st.x, f=st.f, lam=st.lam, status=st.status, nit=st.nit, nfev=st.nfev)

    def array_loss(self, params, batch, fe=None):
        torch = self.torch
        X = self.dev(params).reshape(-1, self.NP)
        B = X.shape[0]
        keep, ba = self._batch_args(X, batch, fe)
        z = lambda: torch.zeros((B, L.NBINS), dtype=torch.float64, device=self.device)
        sums = torch.zeros((B, 3), dtype=torch.float64, device=self.device)
        sqe, sqi, E, I = z(), z(), z(), z()
        self._sync_stream()
        rc = self.lib.tsff_array_loss(self.h, *ba, self._ptr(sums), self._ptr(sqe), self._ptr(sqi), self._ptr(E), self._ptr(I))
        L.check(self.lib, self.h, rc)
        return sums, sqe, sqi, E, I

    def set_denominator_mode(self, mode: int):
        """0: constant denominators (fit loss); 2: |data| + 1e-10 per sample (the reference's Hessian loss)."""
        L.check(self.lib, self.h, self.lib.tsff_set_option(self.h, L.OPT_DENOM_MODE, int(mode)))

    def set_launch_plan(self, plan: int):
        """Bit mask (TSFF_OPT_LAUNCH_PLAN).  0: automatic (one 256-thread workgroup per (lineout, feature) when two fit a
        CU; loss + gradient by the one-sweep kernel where its restrictions hold); bit 0: never interleave the features;
        bit 1: always the two-sweep kernel; bit 2: never three forward-only workgroups per CU."""
        L.check(self.lib, self.h, self.lib.tsff_set_option(self.h, L.OPT_LAUNCH_PLAN, int(plan)))

    def last_launch(self) -> list:
        """Names of the kernels the most recent library call on this engine enqueued, in launch order (tsff_last_launch),
        spelled like their demangled device symbols, e.g. ["k_fused_prep<1>", "k_spectrum_fused<1, 0, false, true>", ...]."""
        s = self.lib.tsff_last_launch(self.h).decode()
        return s.split(";") if s else []

    def set_dlm_blocks(self, n: int):
        """TSFF_OPT_DLM_BLOCKS: column blocks of the pipelined DLM step (per-lineout tables of block i + 1 on a second stream while
        the one-sweep kernel works on block i).  0 / 1: off (default: measured slower on gfx950), n: n blocks.  Same bits."""
        L.check(self.lib, self.h, self.lib.tsff_set_option(self.h, L.OPT_DLM_BLOCKS, int(n)))

    def fp64_fma_peak_tflops(self) -> float:
        """Measured FP64 vector FMA rate of this device (micro-benchmark, TFLOP/s)."""
        v = C.c_double()
        L.check(self.lib, self.h, self.lib.tsff_fp64_fma_peak(self.h, C.byref(v)))
        return float(v.value)

    def l1_read_peak_tbps(self) -> float:
        """Measured vector-L1 read rate of this device (micro-benchmark, TB/s): the roof of the 2-D sampler for tables read
        through L1/L2."""
        v = C.c_double()
        L.check(self.lib, self.h, self.lib.tsff_l1_read_peak(self.h, C.byref(v)))
        return float(v.value)

    def fp64_mfma_peak_tflops(self) -> float:
        """Measured FP64 matrix-core (v_mfma_f64_16x16x4_f64) rate of this device (micro-benchmark, TFLOP/s)."""
        v = C.c_double()
        L.check(self.lib, self.h, self.lib.tsff_fp64_mfma_peak(self.h, C.byref(v)))
        return float(v.value)

    def enable_timing(self, ring: int = 256):
        """Record one HIP event pair around every main-kernel launch (ring of ``ring`` launches)."""
        L.check(self.lib, self.h, self.lib.tsff_enable_timing(self.h, int(ring)))

    def kernel_times_ms(self, max_n: int = 65536) -> np.ndarray:
        buf = (C.c_float * max_n)()
        n = C.c_int32()
        L.check(self.lib, self.h, self.lib.tsff_kernel_times(self.h, buf, max_n, C.byref(n)))
        return np.array(buf[: n.value], dtype=np.float64)
