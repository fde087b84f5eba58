"""Outputs of the 2-D point kernels for a library-against-library comparison (TSFF_LIBRARY): the plain and the saving forward, the
adjoint that samples for itself and the one that reads the forward's projection records, with the table adjoint.

usage: TSFF_LIBRARY=<libtsff.so> python scripts/ff2d_dump.py OUT_DIR [nv ...]     (one process per library, then compare the .npy
files; nv ...: only the cases of these table sizes)

Deck and inputs of tests/test_gpu_parity.py::test_form_factor_2d_grad_finite_differences.  Cases (nv, n_ion, G): table in LDS with four
and two parts per column (48; 100, whose LDS pitch residue is 2), through L1/L2 with the rolling window (132; 133: odd) and with
several columns per thread (257); one and two ion species, three gradient points for one LDS case.
P and grad_phys come out of fixed-order reductions (the same bits run to run); grad_fe2d out of LDS atomics whose order is not fixed."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import decks  # noqa: E402
import util  # noqa: E402
from oracle import tsadar_oracle as orc  # noqa: E402
from tsadar_amd.engine import Engine  # noqa: E402

CASES = [(48, 1, 1), (48, 2, 3), (100, 1, 1), (100, 2, 1), (132, 1, 1), (132, 2, 1), (133, 1, 1), (133, 2, 1), (257, 1, 1), (257, 2, 1)]


def fe2d(nv):
    vx = orc.velocity_grid(nv)
    X, Y = np.meshgrid(vx, vx, indexing="ij")
    f = np.exp(-((X / 1.3) ** 2 + (Y / 0.8) ** 2) ** 1.4 / 2) + 0.05 * np.exp(-((X - 2.0) ** 2 + (Y + 1.0) ** 2))
    return f / (f.sum() * (vx[1] - vx[0]) ** 2)


def main(out, only=()):
    os.makedirs(out, exist_ok=True)
    for nv, n_ion, G in CASES:
        if only and nv not in only:
            continue
        cfg = decks.deck_fit(n_ion=n_ion)
        if G > 1:
            g = cfg["parameters"]["general"]
            g["Te_gradient"].update(val=6.0, num_grad_points=G)
            g["ne_gradient"].update(val=9.0, num_grad_points=G)
        B = 2
        sa = dict(sa=np.array([35.0, 60.0, 110.0]), weights=np.ones((B, 3)) / 3)
        eng = Engine(cfg, sa)
        normed = util.random_lineouts(cfg, B, seed=67, ranges=dict(ud=(-1.5, 1.5)))
        phys = orc.physical_params(cfg["parameters"], normed, True)
        phys["ud"] = np.array([0.8, -1.1])
        X = util.normed_to_matrix(phys, n_ion)
        fe2 = fe2d(nv)
        ud_ang, va_ang = 25.0, -40.0
        rng = np.random.default_rng(8)
        for feature in (0, 1):
            tag = os.path.join(out, f"nv{nv}_ion{n_ion}_G{G}_f{feature}_")
            P0 = eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang)
            Pbar = torch.as_tensor(rng.standard_normal(tuple(P0.shape)), device=P0.device) / P0.abs().mean()
            np.save(tag + "P.npy", P0.cpu().numpy())
            gp, gf = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang)
            np.save(tag + "grad_phys.npy", gp.cpu().numpy())
            np.save(tag + "grad_fe2d.npy", gf.cpu().numpy())
            if nv <= 256:
                P1 = eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang, save=True)
                np.save(tag + "P_save.npy", P1.cpu().numpy())
                gp3, gf3 = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang, use_saved=True)
                np.save(tag + "grad_phys_saved.npy", gp3.cpu().numpy())
                np.save(tag + "grad_fe2d_saved.npy", gf3.cpu().numpy())
        torch.cuda.synchronize()
        print(f"nv {nv} n_ion {n_ion} G {G}: written", flush=True)
    print("library", os.environ.get("TSFF_LIBRARY", "in-tree"))


if __name__ == "__main__":
    main(sys.argv[1], [int(a) for a in sys.argv[2:]])
