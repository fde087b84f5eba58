"""tsff_angular_fit / Engine.angular_fit / loops.angular_loop: the reference's angular loop (angular_optax,
inverse/loops.py:167-275) run on the device, against a host restatement of that loop body over LossFunction.vg_loss with
tree.Adam or tree.RMSProp.

The device and the host evaluate the same kernels for the forward and the adjoints; the loss, its reduction and the chain
rule reduce in another order on the device, so the two agree to rounding: 1e-9 relative on the loss of every epoch and 1e-8
on the final and best leaves."""
import copy
import inspect

import numpy as np
import pytest

import decks
import test_arb1v_generator_device as arb1v_deck
import test_sph_generator_device as sph_deck
from tsadar_amd import _lib as L
from util import _angular_sa, _device, _host_loop, _rel, _stage_records

N_EPOCHS = 30
ROWS = (10, 110)   # lineouts of the 128 x 256 CCD (as test_angular_optax_loop_like_reference)
SPH_FE = {"active": False, "dim": 2, "type": "sphericalharmonic", "nvx": 48,
          "params": {"flm_type": "mora-yahi", "init_m": 2.2, "LTx": 225000.0, "LTy": 400000.0, "Nl": 1, "nvr": 48}}


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_rmsprop_matches_the_restated_formula():
    from tsadar_amd import tree

    rng = np.random.default_rng(5)
    diff = tree.DiffParams([(("electron", "Te"), 0), (("electron", "fval"), tree.FVAL2D_SLOT)], [rng.normal(size=1), rng.normal(size=(4, 4))])
    opt = tree.RMSProp(0.03)
    state = opt.init(diff)
    nu = [np.zeros(1), np.zeros((4, 4))]
    x = [v.copy() for v in diff.values]
    for _ in range(5):
        g = tree.DiffParams(diff.slots, [rng.normal(size=v.shape) for v in diff.values])
        upd, state = opt.update(g, state)
        diff = tree.apply_updates(diff, upd)
        for k, gk in enumerate(g.values):
            nu[k] = 0.9 * nu[k] + (1 - 0.9) * gk * gk
            x[k] = x[k] + (-0.03 * gk / np.sqrt(nu[k] + 1e-8))
            assert np.array_equal(state.values[k], nu[k])
            assert np.array_equal(diff.values[k], x[k])


def test_angular_loop_has_the_reference_signature():
    from tsadar_amd import loops

    names = list(inspect.signature(loops.angular_loop).parameters)
    assert names[:3] == ["config", "all_data", "sa"], names


def _refused(cfg, **kw):
    """angular_loop must refuse before it creates an engine: on a machine without a device, creating one raises TsffError."""
    from tsadar_amd import loops

    with pytest.raises(NotImplementedError):
        loops.angular_loop(cfg, {}, {}, **kw)


def test_angular_loop_refuses_before_device_work():
    cfg = decks.deck_angular(2, 48, (128, 256), *ROWS)
    for method in ("sgd", "lbfgs", "adamw"):
        c = copy.deepcopy(cfg)
        c["optimizer"]["method"] = method
        _refused(c)
    c = copy.deepcopy(cfg)
    c["optimizer"]["method"] = "adam"
    c["data"]["shotnum"] = [101675, 101676]
    _refused(c)
    c = copy.deepcopy(cfg)
    c["optimizer"]["method"] = "rmsprop"
    _refused(c, distributed=True)
    c = copy.deepcopy(cfg)
    c["optimizer"]["method"] = "adam"
    c["parameters"]["electron"]["fe"] = dict(SPH_FE, active=True)
    _refused(c)
    c = decks.deck_angular(1, 64, (128, 256), *ROWS)
    c["optimizer"]["method"] = "adam"
    c["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": 64, "params": {"init_m": 2.0}}
    _refused(c)
    # the refused calls left the config as it was (the reference's mutations come after the checks)
    assert cfg["data"]["lineouts"]["start"] == ROWS[0] and c["data"]["lineouts"]["start"] == ROWS[0]


def _fe_deck(dim, nvx, fe=None):
    cfg = decks.deck_angular(dim, nvx, (128, 256), *ROWS)
    if fe is not None:
        cfg["parameters"]["electron"]["fe"] = copy.deepcopy(fe)
    return cfg


# kind -> (deck, generator, length of the leaves' tail, size of gen_data (the layout's for a trained SphericalHarmonics), the
# spec fields the generator adds): the rows of tsff_angular_fit's table (include/tsff.h) for the decks of the GPU tests
ANGLES = {"ud_angle", "va_angle"}
SPH_META = {"sph_type", "n_harm", "nv", "nvr", "n_gen"}
GENERATORS = {
    "dlm": (lambda: _fe_deck(1, 64), L.ANG_DLM, 0, 64 * 31 + 31, set()),
    "arb": (lambda: _fe_deck(2, 48), L.ANG_ARB2V, 48 * 48, None, ANGLES | {"learn_log"}),
    "sph": (lambda: _fe_deck(2, 48, SPH_FE), L.ANG_TABLE2D, 0, 48 * 48, ANGLES),
    "mora-yahi": (lambda: _fe_deck(2, 48, sph_deck._fe_cfg("mora-yahi", 48, 48)), L.ANG_SPH, 3, "layout", ANGLES | SPH_META),
    "free": (lambda: _fe_deck(2, 48, sph_deck._fe_cfg("arbitrary", 48, 40)), L.ANG_SPH, 2 * 2 * 40 + 1, "layout", ANGLES | SPH_META),
    "arb1v": (lambda: _fe_deck(1, arb1v_deck.NV, arb1v_deck.FE), L.ANG_ARB1V, arb1v_deck.NV, 2 * arb1v_deck.NV**2, set()),
}


@pytest.mark.parametrize("kind", list(GENERATORS))
def test_generator_description(kind):
    """loops._generator, without a device: the generator's code, the sizes of its leaves and constants, the spec fields it adds,
    and the write-back of a perturbed tail, read again bit for bit."""
    from tsadar_amd import ThomsonParams, loops
    from tsadar_amd import distribution as Dist

    deck, code, n_tail, n_data, keys = GENERATORS[kind]
    cfg = deck()
    tp = ThomsonParams(cfg["parameters"], num_params=1, batch=False, activate=True)
    g = loops._generator(cfg, tp, True)
    assert g.code == code and g.tail.shape == (n_tail,) and g.tail.dtype == np.float64
    if n_data == "layout":
        n_data = Dist.sph_gen_layout(*(g.spec[k] for k in ("sph_type", "n_harm", "nv", "nvr")))["size"]
        assert g.spec["n_gen"] == n_tail and g.spec["nv"] == 48
    assert (g.gen_data is None) if n_data is None else (g.gen_data.size == n_data and g.gen_data.dtype == np.float64)
    assert set(g.spec) == keys, g.spec
    other = tp.copy()
    tail = g.tail + 0.01 * np.random.default_rng(1).standard_normal(n_tail)
    g.write_back(other, tail)
    assert np.array_equal(loops._generator(cfg, other, True).tail, tail)
    assert np.array_equal(loops._generator(cfg, tp, True).tail, g.tail), "the write-back touched the original"
    assert (set(g.state_extra(other)) == {"flm"}) if code == L.ANG_SPH else (g.state_extra(other) == {})
    if code in (L.ANG_SPH, L.ANG_ARB1V):   # the two generators that train_generator switches on
        assert loops._generator(cfg, tp, False) is None


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _case(kind, method, lr=0.002, n_epochs=N_EPOCHS, noise=0.0, offset=0.0, loss_method="l2", truth_start=False, noise_e=0.0):
    """(config, all_data, sa): a 128 x 256 ARTS image made from a 'truth' plasma (another Te and, for Arbitrary2V, another
    table order) and a deck that starts elsewhere (truth_start: at the truth).  kind "ions2": the DLM deck with a second ion
    species whose Ti is tied to ion-1's, which is a leaf.  noise_e: the constant background of the fit (noiseE)."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L
    from tsadar_amd import distribution as Dist
    from tsadar_amd.loss_function import LossFunction

    if kind in ("dlm", "ions2"):
        cfg = decks.deck_angular(1, 64, (128, 256), *ROWS)
        if kind == "ions2":
            P = cfg["parameters"]
            P["ion-1"]["Ti"]["active"] = True
            P["ion-1"]["fract"]["val"] = 0.6
            P["ion-2"] = {"Ti": dict(P["ion-1"]["Ti"], val=0.3, active=False, same=True), "Z": dict(P["ion-1"]["Z"], val=1.0, active=False),
                          "A": {"val": 1.0, "active": False}, "fract": {"val": 0.4, "active": False}}
    else:
        cfg = decks.deck_angular(2, 48, (128, 256), *ROWS)
        if kind == "sph":
            cfg["parameters"]["electron"]["fe"] = copy.deepcopy(SPH_FE)
    cfg["other"]["ang_res_unit"] = 1
    opt = cfg["optimizer"]
    opt.update(method=method, learning_rate=lr, num_epochs=n_epochs, loss_method=loss_method, save_state=False, save_state_freq=5)
    sa = _angular_sa(cfg)
    rows = ROWS[1] - ROWS[0]
    batch = dict(e_data=np.ones((rows, 256)), i_data=np.zeros((rows, 256)), e_amps=np.ones((rows, 1)), i_amps=np.zeros(rows),
                 noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    truth = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    if not truth_start:
        truth.X[0, L.P_TE] -= 0.3
        if kind in ("dlm", "ions2"):
            truth.X[0, L.P_M] += 0.4
        if kind == "arb":
            truth.fval2d = Dist.arbitrary_2v_init(3.2, 48, truth.learn_log)
    E = LossFunction(copy.deepcopy(cfg), sa, batch).ts_diag(truth, batch)[0]
    rng = np.random.default_rng(3)
    E = E * (1.0 + noise * rng.standard_normal(E.shape)) + offset
    e_data = np.ones((128, 256))
    e_data[ROWS[0]:ROWS[1]] = E
    all_data = dict(e_data=e_data, e_amps=np.ones((128, 1)), i_data=np.zeros((128, 256)), i_amps=np.zeros(128),
                    noiseE=np.full((128, 256), float(noise_e)), noiseI=np.zeros((128, 256)))
    return cfg, all_data, sa


def _leaves(tp):
    v = tp.X[0]
    return np.concatenate([v, tp.fval2d.ravel()]) if getattr(tp, "fval2d", None) is not None and tp.slots.fval2d_active else v


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("kind", ["dlm", "arb", "sph"])
def test_angular_loop_matches_the_host_loop(torch_mod, kind, method):
    from tsadar_amd import _lib as L

    # (RMSProp takes no bias correction: its first steps are ~3 lr.  At lr 0.002 it oscillates on these decks and the rounding
    # differences of the loss reduction grow from epoch to epoch; at 2e-4 it descends)
    cfg, all_data, sa = _case(kind, method, lr=0.002 if method == "adam" else 2e-4)
    loss_fn = _compare_with_host(cfg, all_data, sa)
    if kind == "dlm":
        assert loss_fn.ts_diag.engine(True).slots.active[L.P_M]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,loss_method", [("dlm", "l1"), ("dlm", "poisson"), ("arb", "l1"), ("ions2", "l2")])
def test_angular_loop_other_losses_and_tied_ions(torch_mod, kind, loss_method):
    """The l1 and poisson branches of the loss (with a constant background noise_e, which poisson needs positive), and the Ti
    tying of the chain rule (two ion species, ion-2's Ti "same" as ion-1's, which is a leaf)."""
    from tsadar_amd import _lib as L

    # (l1's seed is -sign(d - Et): where the residual crosses zero, rounding can put a pixel on either side, and the seed jumps
    # by 2 w / un -- 2e-7 in the loss by epoch 30 on the DLM deck.  Data 1 above the model keep every residual one-signed; the
    # loss is then linear in the image and lam's gradient a near-cancelling sum, so the leaves are held to 1e-8 of max(|x|, 1))
    l1 = loss_method == "l1"
    cfg, all_data, sa = _case(kind, "adam", loss_method=loss_method, noise_e=0.05, offset=1.0 if l1 else 0.0)
    loss_fn = _compare_with_host(cfg, all_data, sa, leaf_floor=1.0 if l1 else 0.0)
    if kind == "ions2":
        sm = loss_fn.ts_diag.engine(True).slots
        assert sm.n_ion == 2 and sm.ti_same[1] and sm.active[L.P_ION0 + L.ION_TI]


def _compare_with_host(cfg, all_data, sa, leaf_floor=0.0):
    host = _host_loop(cfg, all_data, sa)
    best, epoch_loss, loss_fn, info = _device(cfg, all_data, sa)
    n = len(host["losses"])
    assert info["stopped_after"] == host["stopped"]
    assert _rel(info["loss_hist"][:n], host["losses"]) < 1e-9, (info["loss_hist"][:n], host["losses"])
    assert abs(epoch_loss - host["epoch_loss"]) <= 1e-9 * abs(host["epoch_loss"])
    assert host["best"] != {} and best != {}
    assert _rel(_leaves(best), _leaves(host["best"]), leaf_floor) < 1e-8
    assert _rel(info["leaves"], _leaves(host["final"]), leaf_floor) < 1e-8
    assert host["losses"][-1] < host["losses"][0]
    return loss_fn


@pytest.mark.gpu
def test_angular_loop_early_stop_and_no_improvement(torch_mod):
    # from the truth of a noisy image with a small step, every improvement is below 1e-6: the stop after six of them
    cfg, all_data, sa = _case("dlm", "adam", lr=1e-5, n_epochs=40, noise=0.01, truth_start=True)
    host = _host_loop(cfg, all_data, sa)
    best, epoch_loss, _, info = _device(cfg, all_data, sa, chunk=5)
    assert host["stopped"] is not None and info["stopped_after"] == host["stopped"], (host["stopped"], info["stopped_after"])
    assert np.isnan(info["loss_hist"][host["stopped"] + 1:]).all()
    assert _rel(_leaves(best), _leaves(host["best"])) < 1e-8
    assert abs(epoch_loss - host["epoch_loss"]) <= 1e-9 * abs(host["epoch_loss"])
    # an image 150 above the model under log-cosh: no epoch beats 100.0, the best weights stay the dict they started as
    cfg, all_data, sa = _case("dlm", "rmsprop", lr=1e-4, n_epochs=6, offset=150.0, loss_method="log-cosh")
    host = _host_loop(cfg, all_data, sa)
    best, epoch_loss, _, info = _device(cfg, all_data, sa)
    assert host["best"] == {} and best == {}
    assert min(host["losses"]) > 100.0 and abs(epoch_loss - host["epoch_loss"]) <= 1e-9 * abs(host["epoch_loss"])


@pytest.mark.gpu
def test_angular_loop_save_state_epochs(torch_mod):
    cfg, all_data, sa = _case("arb", "adam", n_epochs=12)
    cfg["optimizer"].update(save_state=True, save_state_freq=3)
    host = _host_loop(cfg, all_data, sa)
    states = {}
    _device(cfg, all_data, sa, chunk=5, states=states)
    assert sorted(states) == sorted(host["states"]) == [0, 3, 6, 9]
    for i, s in states.items():
        h = host["states"][i]
        for sp in h:
            for k in h[sp]:
                assert _rel(s[sp][k], h[sp][k]) < 1e-8, (i, sp, k)


@pytest.mark.gpu
def test_angular_loop_chunks_are_bit_identical(torch_mod):
    cfg, all_data, sa = _case("dlm", "adam", n_epochs=20)
    runs = [_device(cfg, all_data, sa, chunk=c) for c in (1, 7, 20)]
    for best, epoch_loss, _, info in runs[1:]:
        assert np.array_equal(info["loss_hist"], runs[0][3]["loss_hist"])
        assert np.array_equal(info["leaves"], runs[0][3]["leaves"])
        assert np.array_equal(best.X, runs[0][0].X) and epoch_loss == runs[0][1]


# kind -> (the generator's kernels after k_ang_leaves, its kernels after k_ang_chain): TABLE2D, DLM, ARB2V, SPH, ARB1V
LAUNCHES = {"sph": ([], []), "dlm": ([], []), "arb": ([], []), "sphtrain": (["k_sph_table"], ["k_sph_vjp"]),
            "arb1v": (["k_arb1v_matvec", "k_arb1v_point"], ["k_arb1v_point", "k_arb1v_matvec"])}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(LAUNCHES))
def test_angular_fit_launch_record(torch_mod, monkeypatch, kind):
    """One epoch's record = k_ang_leaves, the generator's forward kernels, then what the stand-alone entry points enqueue (form
    factor, ATS chain, loss, ATS adjoint, form-factor adjoint), k_ang_chain, the generator's adjoint kernels and k_ang_opt --
    the same list every epoch (arb1v: with the timing ring on as without)."""
    from tsadar_amd import _lib as L
    from tsadar_amd.engine import Engine

    gen_fwd, gen_adj = LAUNCHES[kind]
    two_d = kind not in ("dlm", "arb1v")
    if kind == "sphtrain":
        cfg, all_data, sa = sph_deck._case("mora-yahi", "rmsprop", n_epochs=3)
    elif kind == "arb1v":
        cfg, all_data, sa = arb1v_deck._case("rmsprop", arb1v_deck.LR["rmsprop"])
        cfg = copy.deepcopy(cfg)
        cfg["optimizer"]["num_epochs"] = 3
        fit = Engine.angular_fit

        def timed(self, *a, **kw):
            self.enable_timing(64)
            return fit(self, *a, **kw)

        monkeypatch.setattr(Engine, "angular_fit", timed)
    else:
        cfg, all_data, sa = _case(kind, "rmsprop" if kind == "arb" else "adam", n_epochs=3)
    _, _, loss_fn, _ = _device(cfg, all_data, sa, chunk=3, train_generator=kind in ("sphtrain", "arb1v"))
    monkeypatch.undo()
    eng = loss_fn.ts_diag.engine(True)
    rec = eng.last_launch()
    assert len(rec) % 3 == 0 and rec[0].startswith("k_ang_leaves<")
    per = rec[: len(rec) // 3]
    assert rec == per * 3, rec
    fwd, spec, adj, grad = _stage_records(eng, cfg, two_d, want_gfe=kind != "sph")
    assert all(len(r) > 0 for r in (fwd, spec, adj, grad))
    nf, na = len(gen_fwd), len(gen_adj)
    assert per[0].startswith("k_ang_leaves<") and per[1 : 1 + nf] == gen_fwd, per
    assert per[1 + nf : -2 - na] == fwd + spec + ["k_ang_loss", "k_ang_loss_sum"] + adj + grad, (per, fwd, spec, adj, grad)
    assert per[-2 - na].startswith("k_ang_chain<") and per[-1 - na :] == gen_adj + ["k_ang_opt"], per
    if not two_d:   # the 1-D decks (m a leaf, or fval trained): the adjoint with its f_e tail
        assert any(r.startswith("k_form_factor<") for r in per) and "k_fe_adjoint" in per and "k_fe_adjoint" in grad, per
    if kind != "arb":
        return
    for k in ("k_form_factor_2d<", "k_ats_resunit", "k_ang_loss", "k_ats_resunit_adj", "k_form_factor_2d_adj<", "k_ang_chain<", "k_ang_opt"):
        assert any(r.startswith(k) for r in per), (k, per)
    # a refused call enqueues nothing
    x = eng.dev(np.zeros(eng.NP))
    spec = dict(generator=L.ANG_DLM, nv=48, active_slots=[L.P_TE, L.P_TE], loss_method=0, un=1.0, dvx=0.25, method=L.ANG_ADAM,
                lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
    z = eng.dev(np.zeros(100 * 256)).reshape(100, 256)
    data = dict(gen_data=eng.dev(np.zeros(48 * 31 + 31)), e_data=z, noise_e=z, wcol=eng.dev(np.zeros(256)), e_amps=eng.dev(np.ones(100)))
    with pytest.raises(L.TsffError):
        eng.angular_fit(x, spec, data, 4)
    assert eng.last_launch() == []


@pytest.mark.gpu
def test_angular_fit_invalidates_saved_projection_records(torch_mod, monkeypatch):
    """The fit runs saving 2-D forwards of its own: a token taken from tsff_form_factor_2d_save before the fit is stale after it."""
    import ctypes as C

    from tsadar_amd import ThomsonParams
    from tsadar_amd.engine import Engine

    cfg, all_data, sa = _case("arb", "adam", n_epochs=1)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    phys, fe2 = tp.physical_matrix(), np.ascontiguousarray(tp()["electron"]["fe"], dtype=np.float64)
    assert fe2.shape == (48, 48)
    taken = {}
    fit = Engine.angular_fit

    def save_then_fit(self, *a, **kw):
        taken["P"] = self.form_factor_2d(0, phys, fe2, save=True)
        taken.update(self._saved_2d)
        return fit(self, *a, **kw)

    monkeypatch.setattr(Engine, "angular_fit", save_then_fit)
    _, _, loss_fn, _ = _device(cfg, all_data, sa)
    eng = loss_fn.ts_diag.engine(True)
    assert taken["token"] != 0
    torch = eng.torch
    Pbar = torch.ones_like(taken["P"])
    gp = torch.empty((1, eng.NP), dtype=torch.float64, device=eng.device)
    eng._sync_stream()
    rc = eng.lib.tsff_form_factor_2d_grad(eng.h, 0, eng._ptr(taken["phys_d"]), eng._ptr(taken["fe_d"]), 48, 0.0, 0.0, 1, 0, -1,
                                          C.c_uint64(taken["token"]), eng._ptr(Pbar), eng._ptr(gp), None)
    assert rc == -22 and "stale or foreign token" in eng.lib.tsff_last_error(eng.h).decode()
