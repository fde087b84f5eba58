"""The free-form 1-D f_e generator (the reference's Arbitrary1V) on the device: tsff_arb1v_table / tsff_arb1v_table_vjp
(Engine.arb1v_table, arb1v_table_vjp), the TSFF_ANG_ARB1V generator of tsff_angular_fit and
loops.angular_loop(train_generator=True) on a deck with ``fe: {dim: 1, type: arbitrary, active: true}``.

Bounds.  Generator against the host (distribution.arbitrary_1v, arbitrary_1v_vjp), relative to the largest entry: TABLE_BOUND
and VJP_BOUND, ten times the largest difference measured on an MI355X over the sizes below (the figures are in
test_generator_matches_the_host's docstring; the margin covers other seeds), both far inside the 1e-11 they may not exceed.
Adjoint against central differences of the device forward: 1e-6 max(1, |v|), the bound tests/test_host_logic.py holds the host
VJP to.  Loop against the host loop over LossFunction.vg_loss: the bounds tests/test_angular_loop_device.py holds the trained Arbitrary2V table to (1e-9 relative on
every epoch's loss, 1e-8 on the final and best leaves [X[0] | fval], the same early stop)."""
import copy
import functools
import inspect

import numpy as np
import pytest

import decks
import util
from util import _angular_sa, _host_loop, _rel

N_EPOCHS = 30
ROWS = (10, 110)   # lineouts of the 128 x 256 CCD (as tests/test_angular_loop_device.py)
NV = 64
FE = {"active": True, "type": "arbitrary", "dim": 1, "nvx": NV, "params": {"init_m": 2.5}}
SIZES = (8, 50, 64, 256, 320)   # less than a wavefront, no multiple of 64, one wavefront, 64 workgroups, more rows than 256
TABLE_BOUND, VJP_BOUND = 8e-15, 5e-14   # 10 x (7.6e-16, 4.9e-15), the largest measured over SIZES


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_interface_has_the_generator():
    from tsadar_amd import _lib as L
    from tsadar_amd.engine import Engine

    assert L.ANG_ARB1V == 4
    assert "tsff_arb1v_table" in L.EXPORTS and "tsff_arb1v_table_vjp" in L.EXPORTS
    assert callable(Engine.arb1v_table) and callable(Engine.arb1v_table_vjp)
    assert list(inspect.signature(Engine.arb1v_table).parameters)[1:] == ["fval", "gen_data", "dvx", "out"]
    assert list(inspect.signature(Engine.arb1v_table_vjp).parameters)[1:] == ["fval", "gen_data", "fe_bar", "dvx", "out"]
    # the generator needs no field of its own: the spec still ends with the SphericalHarmonics generator's
    assert [f[0] for f in L.TsffAngularSpec._fields_][-4:] == ["sph_type", "n_harm", "nvr", "n_gen"]


@pytest.mark.parametrize("n", [8, 50])
def test_gen_data_is_the_matrix_and_its_transpose(n):
    from tsadar_amd import distribution as Dist

    gd = Dist.arb1v_gen_data(n)
    S = Dist.butterworth_matrix(n)
    assert gd.dtype == np.float64 and gd.shape == (2 * n * n,)
    assert np.array_equal(gd[: n * n].reshape(n, n), S)
    assert np.array_equal(gd[n * n :].reshape(n, n), S.T)


@pytest.mark.parametrize("fe", [dict(FE, active=False), dict(FE, type="spitzer")], ids=["inactive", "unknown-type"])
def test_train_generator_refuses_before_device_work(fe):
    """A free-form 1-D f_e that is not trained and any other 1-D type are refused before the config is mutated and before an
    engine is created (on a machine without a device, creating one raises TsffError, not NotImplementedError)."""
    from tsadar_amd import loops

    cfg = decks.deck_angular(1, NV, (128, 256), *ROWS)
    cfg["optimizer"]["method"] = "adam"
    cfg["parameters"]["electron"]["fe"] = copy.deepcopy(fe)
    before = copy.deepcopy(cfg)
    with pytest.raises(NotImplementedError):
        loops.angular_loop(cfg, {}, {}, train_generator=True)
    assert cfg == before


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng(torch_mod):
    """One engine for the stand-alone generator calls (they use the handle's stream and scratch only)."""
    from tsadar_amd.engine import Engine

    cfg = decks.deck_angular(1, NV, (128, 256), *ROWS)
    return Engine(cfg, _angular_sa(cfg))


@functools.lru_cache(maxsize=None)
def _inputs(nv):
    """(fval, fe_bar, gen_data) of a size: the order-2.5 start plus a seeded perturbation of 0.02, a seeded normal fe_bar."""
    from tsadar_amd import distribution as Dist

    rng = np.random.default_rng(100 + nv)
    fval = Dist.arbitrary_1v_init(2.5, nv) + 0.02 * rng.standard_normal(nv)
    return fval, rng.standard_normal(nv), Dist.arb1v_gen_data(nv)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", SIZES)
def test_generator_matches_the_host(eng, nv):
    """Engine.arb1v_table against distribution.arbitrary_1v and arb1v_table_vjp against distribution.arbitrary_1v_vjp,
    relative to the largest entry (f_e reaches 1e-25 in the tails at nv = 320), the unit integral and bit-reproducibility.
    The difference comes from the order of the sums and from exp against np.power.

    Measured on an MI355X (table, vjp): nv 8: 3.8e-16, 4.9e-15; nv 50: 4.4e-16, 1.5e-15; nv 64: 4.3e-16, 3.1e-16; nv 256: 7.6e-16,
    4.8e-16; nv 320: 6.0e-16, 5.3e-16; the integral of f_e within 2.3e-16 of 1."""
    from tsadar_amd import distribution as Dist

    fval, fe_bar, gd = _inputs(nv)
    want, want_g = Dist.arbitrary_1v(fval), Dist.arbitrary_1v_vjp(fval, fe_bar)
    assert np.all(np.isfinite(want)) and abs(np.sum(want) * 12.0 / nv - 1.0) < 1e-13
    fv, gdd, fb = eng.dev(fval), eng.dev(gd), eng.dev(fe_bar)
    got, again = eng.download(eng.arb1v_table(fv, gdd)), eng.download(eng.arb1v_table(fv, gdd))
    g, g_again = eng.download(eng.arb1v_table_vjp(fv, gdd, fb)), eng.download(eng.arb1v_table_vjp(fv, gdd, fb))
    assert np.array_equal(got, again) and np.array_equal(g, g_again), "two calls on the same input differ"
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(g))
    err = np.max(np.abs(got - want)) / np.max(want)
    err_g = np.max(np.abs(g - want_g)) / np.max(np.abs(want_g))
    print(f"nv {nv}: device table vs host {err:.3e}, device vjp vs host {err_g:.3e}, integral - 1 {np.sum(got) * 12.0 / nv - 1.0:.3e}")
    assert abs(np.sum(got) * 12.0 / nv - 1.0) <= 1e-13
    assert err <= TABLE_BOUND and err_g <= VJP_BOUND, (err, err_g)


@pytest.mark.gpu
def test_adjoint_matches_differences_of_the_device_forward(eng):
    """Independent of the host VJP: central differences of sum(fe_bar * arb1v_table(fval +- 1e-6 e_i)) against arb1v_table_vjp."""
    fval, fe_bar, gd = _inputs(NV)
    gdd = eng.dev(gd)
    v = eng.download(eng.arb1v_table_vjp(fval, gdd, fe_bar))
    for i in (0, 9, 32, 63):
        a, b = fval.copy(), fval.copy()
        a[i] += 1e-6
        b[i] -= 1e-6
        fd = (np.dot(fe_bar, eng.download(eng.arb1v_table(a, gdd))) - np.dot(fe_bar, eng.download(eng.arb1v_table(b, gdd)))) / 2e-6
        print(f"index {i}: vjp {v[i]:.9e}, central difference {fd:.9e}")
        assert abs(fd - v[i]) < 1e-6 * max(1.0, abs(v[i])), (i, fd, v[i])


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments(eng):
    fval, fe_bar, gd = _inputs(8)
    fv, gdd, fb = eng.dev(fval), eng.dev(gd), eng.dev(fe_bar)
    out = eng.torch.empty(8, dtype=eng.torch.float64, device=eng.device)
    eng._sync_stream()
    assert eng.lib.tsff_arb1v_table(eng.h, 8, 1.5, eng._ptr(fv), None, eng._ptr(out)) == -1
    assert eng.lib.tsff_arb1v_table_vjp(eng.h, 8, 1.5, eng._ptr(fv), eng._ptr(gdd), None, eng._ptr(out)) == -1
    for nv in (3, 4097):
        assert eng.lib.tsff_arb1v_table(eng.h, nv, 1.5, eng._ptr(fv), eng._ptr(gdd), eng._ptr(out)) == -2
        assert eng.last_launch() == [] and "nv must be 4 .. 4096" in eng.lib.tsff_last_error(eng.h).decode()
        assert eng.lib.tsff_arb1v_table_vjp(eng.h, nv, 1.5, eng._ptr(fv), eng._ptr(gdd), eng._ptr(fb), eng._ptr(out)) == -2
        assert eng.last_launch() == []


# ---- the fit -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(method, lr):
    """(config, all_data, sa), shared and left unchanged: the small ARTS case of tests/test_angular_loop_device.py with a
    trained free-form 1-D f_e that starts at order 2.5; the 128 x 256 image is made from a 'truth' with Te lowered by 0.3
    (normalised) and fval of order 3.2."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L
    from tsadar_amd import distribution as Dist
    from tsadar_amd.loss_function import LossFunction

    cfg = decks.deck_angular(1, NV, (128, 256), *ROWS)
    cfg["parameters"]["electron"]["fe"] = copy.deepcopy(FE)
    cfg["other"]["ang_res_unit"] = 1
    cfg["optimizer"].update(method=method, learning_rate=lr, num_epochs=N_EPOCHS, loss_method="l2", save_state=False, save_state_freq=5)
    sa = _angular_sa(cfg)
    rows = ROWS[1] - ROWS[0]
    batch = dict(e_data=np.ones((rows, 256)), i_data=np.zeros((rows, 256)), e_amps=np.ones((rows, 1)), i_amps=np.zeros(rows),
                 noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    truth = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    truth.X[0, L.P_TE] -= 0.3
    truth.fval = Dist.arbitrary_1v_init(3.2, NV).reshape(truth.fval.shape)
    E = LossFunction(copy.deepcopy(cfg), sa, batch).ts_diag(truth, batch)[0]
    e_data = np.ones((128, 256))
    e_data[ROWS[0]:ROWS[1]] = E
    all_data = dict(e_data=e_data, e_amps=np.ones((128, 1)), i_data=np.zeros((128, 256)), i_amps=np.zeros(128),
                    noiseE=np.zeros((128, 256)), noiseI=np.zeros((128, 256)))
    return cfg, all_data, sa


# The rates of tests/test_angular_loop_device.py (Adam 0.002, RMSProp 2e-4) are too large for fval: ln f_e moves by
# 2 * 49 * ln 10 * u ~ 150 per unit of fval in the tails (u ~ 0.65 where f_e ~ 1e-21), a hundred times what a scalar leaf does.
# Measured on an MI355X (30 epochs; host loss first -> last, largest per-epoch device-against-host loss difference):
#   Adam    2e-3: 1.561e-2 -> 2.672e-2 (it RISES), 0.57;   5e-4: -> 1.483e-2, 0.41;   2e-4: -> 1.656e-2, 0.11;   5e-5: -> 1.466e-2,
#           8.5e-2;   2e-5: -> 1.503e-2, 6.2e-11 (leaves 1.5e-12);
#   RMSProp 2e-4: -> 1.332e-2, 0.22;   5e-5: -> 1.419e-2, 0.13;   2e-5: -> 1.392e-2, every epoch below the one before, 4.8e-12
#           (leaves 3.5e-12);   5e-6: -> 1.503e-2 but not monotone, 7.0e-6;   2e-6: -> 1.512e-2, monotone, 2.1e-12.
# At every rate the two loops agree to 1e-12 in the first epoch and to 1e-10 for the first three; where the loss does not fall
# steadily the difference then grows by one to three orders per epoch (an unstable trajectory amplifies the rounding of the
# loss reduction, as that file notes for RMSProp at 0.002).  So the rates are lowered, as its comment does: Adam a hundredfold
# and RMSProp tenfold, to rates at which the host loss descends.
LR = {"adam": 2e-5, "rmsprop": 2e-5}


def _leaves(tp):
    return np.concatenate([tp.X[0], tp.fval.ravel()])


_device = functools.partial(util._device, train_generator=True)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_trained_fval_matches_the_host_loop(torch_mod, method):
    from tsadar_amd import _lib as L
    from tsadar_amd import distribution as Dist

    cfg, all_data, sa = _case(method, LR[method])
    host = _host_loop(cfg, all_data, sa)
    best, epoch_loss, loss_fn, info = _device(cfg, all_data, sa)
    n = len(host["losses"])
    print(method, "host losses first / last:", host["losses"][0], host["losses"][-1], "stopped:", host["stopped"], info["stopped_after"])
    assert info["stopped_after"] == host["stopped"]
    print(method, "loss:", _rel(info["loss_hist"][:n], host["losses"]), "best leaves:", _rel(_leaves(best), _leaves(host["best"])),
          "final leaves:", _rel(info["leaves"], _leaves(host["final"])))
    assert _rel(info["loss_hist"][:n], host["losses"]) < 1e-9, (info["loss_hist"][:n], host["losses"])
    assert abs(epoch_loss - host["epoch_loss"]) <= 1e-9 * abs(host["epoch_loss"])
    assert host["best"] != {} and best != {}
    assert info["leaves"].shape == (loss_fn.ts_diag.engine(True).NP + NV,)
    assert _rel(_leaves(best), _leaves(host["best"])) < 1e-8
    assert _rel(info["leaves"], _leaves(host["final"])) < 1e-8
    assert host["losses"][-1] < host["losses"][0]
    # fval moved, m is no leaf of this deck, and the fit used the new generator
    assert best.fval.shape == (1, NV) and np.max(np.abs(best.fval[0] - Dist.arbitrary_1v_init(2.5, NV))) > 1e-5
    assert not loss_fn.ts_diag.engine(True).slots.active[L.P_M]
    assert "k_arb1v_matvec" in loss_fn.ts_diag.engine(True).last_launch()


@pytest.mark.gpu
def test_chunks_are_bit_identical(torch_mod):
    cfg, all_data, sa = _case("adam", LR["adam"])
    runs = [_device(cfg, all_data, sa, chunk=c) for c in (1, 7, 30)]
    for best, epoch_loss, _, info in runs[1:]:
        assert np.array_equal(info["loss_hist"], runs[0][3]["loss_hist"])
        assert np.array_equal(info["leaves"], runs[0][3]["leaves"])
        assert np.array_equal(best.X, runs[0][0].X) and np.array_equal(best.fval, runs[0][0].fval)
        assert epoch_loss == runs[0][1]
    assert np.isfinite(runs[0][3]["loss_hist"]).all()


@pytest.mark.gpu
def test_saved_states_carry_the_best_fe(torch_mod):
    cfg, all_data, sa = _case("adam", LR["adam"])
    cfg = copy.deepcopy(cfg)
    cfg["optimizer"].update(save_state=True, save_state_freq=3, num_epochs=12)
    host = _host_loop(cfg, all_data, sa)
    states = {}
    _device(cfg, all_data, sa, chunk=5, states=states)
    assert sorted(states) == sorted(host["states"]) and len(states) > 0
    fs = []
    for i, s in states.items():
        h = host["states"][i]
        a, b = np.asarray(s["electron"]["f"]), np.asarray(h["electron"]["f"])
        assert a.shape == b.shape == (NV,)
        assert np.max(np.abs(a - b)) <= 1e-8 * np.max(np.abs(b)), i
        fs.append(a)
        for sp in h:
            for k in h[sp]:
                if k != "f":
                    assert _rel(s[sp][k], h[sp][k]) < 1e-8, (i, sp, k)
    assert len(fs) < 2 or not np.array_equal(fs[0], fs[-1]), "every state carries the same f_e"


@pytest.mark.gpu
def test_fit_refusals_enqueue_nothing(torch_mod):
    from tsadar_amd import _lib as L
    from tsadar_amd import distribution as Dist

    cfg, all_data, sa = _case("adam", LR["adam"])
    cfg = copy.deepcopy(cfg)
    cfg["optimizer"]["num_epochs"] = 1
    _, _, loss_fn, _ = _device(cfg, all_data, sa)
    eng = loss_fn.ts_diag.engine(True)
    rows, nJ = eng._ats_shape
    z = eng.dev(np.zeros(rows * nJ)).reshape(rows, nJ)
    good = dict(generator=L.ANG_ARB1V, nv=NV, active_slots=[L.P_TE], loss_method=0, un=1.0, dvx=12.0 / NV, method=L.ANG_ADAM, lr=1e-3,
                b1=0.9, b2=0.999, eps=1e-8)
    data = dict(gen_data=eng.dev(Dist.arb1v_gen_data(NV)), e_data=z, noise_e=z, wcol=eng.dev(np.zeros(nJ)), e_amps=eng.dev(np.ones(rows)))
    x48, x64 = np.zeros(eng.NP + 48), np.zeros(eng.NP + NV)
    for x, spec, d, code, reason in ((x64, dict(good, active_slots=[L.P_TE, L.P_M]), data, -2, "DLM order m"),
                                     (x48, dict(good, nv=48), data, -1, "handle's nvx"),
                                     (x64, good, dict(data, gen_data=None), -1, "gen_data missing")):
        with pytest.raises(L.TsffError, match=f"libtsff error {code}:") as e:
            eng.angular_fit(eng.dev(x), spec, d, 2)
        assert reason in str(e.value) and reason in eng.lib.tsff_last_error(eng.h).decode(), str(e.value)
        assert eng.last_launch() == []
