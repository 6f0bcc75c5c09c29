"""CPU: the yardstick of tests/test_hip_eqff_chain.py (tests/eqff_util.py) proved without a GPU -- the fp64 chain agrees with
the oracle's EQFF and its hand-written input-gradient with autograd; a CPU model of each arithmetic stays inside the
per-atom bounds on every input set the GPU test launches; the bounds reject what they should."""
import pytest
import torch

from tests import eqff_util as U


def test_reference_matches_oracle_eqff_and_autograd():
    from oracle import gotennet_oracle as orc
    F = 16
    d = U.make(F, 5, 8, seed=1)
    d["Xp"] = d["X"].clone()                        # W_vu = identity: the oracle's own X_p is X, bit for bit
    sd = {"e.W_vu.weight": torch.eye(F, dtype=torch.float64), "e.gamma_m.0.weight": d["W0"].double(),
          "e.gamma_m.0.bias": d["b0"].double(), "e.gamma_m.1.weight": d["W1"].double(), "e.gamma_m.1.bias": d["b1"].double()}
    h1, X1 = orc.eqff(sd, {"n_atom_basis": F, "epsilon": d["eps"]}, "e.", d["h"].double(), d["X"].double())
    r = U.forward_ref(d)
    assert torch.allclose(r["h1"], h1, rtol=1e-13, atol=1e-13) and torch.allclose(r["X1"], X1, rtol=1e-13, atol=1e-13)
    for dd in (d, U.make(128, 9, 15), U.make(128, 17, 8, hostile="spread")):
        r = U.forward_ref(dd)
        b = U.backward_ref(dd, r["mm"], r["ctx"], r["pre"])
        g_Xp, g_h1 = U.backward_autograd(dd)
        assert torch.allclose(b["gXp"], g_Xp, rtol=1e-9, atol=1e-30) and torch.allclose(b["gh1"], g_h1, rtol=1e-9, atol=1e-30)


def _model(op, W, b, arith):
    """One product as the arithmetic sees its operand (f16x2: one exponent per 8-atom tile; split: all of fp32), result
    rounded to fp32."""
    a = U.emulate_f16x2(op) if arith == "f16x2" else op.double()
    return (a @ W.double().t() + U.bias(b)).float()


def _inputs():
    return [U.make(F, N, D) for F, N, D in U.SHAPES] + [U.make(F, 17, 8, hostile="spread") for F in (128, 256)]


@pytest.mark.parametrize("arith", ["f16x2", "split"])
def test_arithmetic_model_is_within_the_bounds(arith):
    worst = dict(p1=0.0, p2=0.0, gXp=0.0, gh1=0.0)
    spread_seen = False
    for d in _inputs():
        F = d["F"]
        r = U.forward_ref(d)
        ctx = r["ctx"].float()
        pre = _model(ctx, d["W0"], d["b0"], arith)
        hid = U.SILU(pre.double()).float()
        mm = _model(hid, d["W1"], d["b1"], arith)
        for name, C, op, W, b in (("p1", pre, ctx, d["W0"], d["b0"]), ("p2", mm, hid, d["W1"], d["b1"])):
            err, bet, dd = U.product_check(C, op, W, b, arith)
            assert bool((err <= bet).all()), (name, float((err / bet).max()))
            near = dd <= U.NEAR_D
            assert float(err[near].max()) < U.NEAR
            worst[name] = max(worst[name], float((err / bet).max()))
            if arith == "f16x2" and d["hostile"] == "spread" and name == "p1":
                # not vacuous: the atoms the bound loosens are the atoms that need it
                assert bool((dd > 28).any()) and float(err[dd > 28].max()) > float(err[near].max())
                spread_seen = True
        # backward on the saved tensors of this forward
        b = U.backward_ref(d, mm, ctx, pre)
        E_gXp, E_gh1 = U.backward_bounds(d, b, mm, ctx, pre, arith)
        gm = b["gm"].float()
        P = _model(gm, d["W1"].t(), None, arith)
        v = (P * U.dsilu(pre)).float()
        gctx = _model(v, d["W0"].t(), None, arith)
        gh1 = d["gh"] + gctx[:, :F]
        gXp = d["gX"] * mm[:, None, F:] + (gctx[:, F:] / ctx[:, F:])[:, None, :] * d["Xp"]
        for name, C, ref, bnd in (("gXp", gXp, b["gXp"], E_gXp), ("gh1", gh1, b["gh1"], E_gh1)):
            ok = bnd > 0
            assert bool(((C.double() - ref).abs() <= bnd).all()), name
            worst[name] = max(worst[name], float(((C.double() - ref).abs()[ok] / bnd[ok]).max()))
        # not vacuous: ONE hidden channel lost from the second product of the last (ordinary) atom breaks both bounds
        a, j = d["N"] - 1, int(b["v"][d["N"] - 1].abs().argmax())
        lost = b["gctx"][a] - b["v"][a, j] * d["W0"].double()[j]
        assert bool(((lost[:F] - b["gctx"][a, :F]).abs() > E_gh1[a]).any())
        lost_gXp = d["gX"][a].double() * mm[a, F:].double() + (lost[F:] / ctx[a, F:].double()) * d["Xp"][a].double()
        assert bool(((lost_gXp - b["gXp"][a]).abs() > E_gXp[a]).any())
    assert spread_seen or arith == "split"
    print(f"{arith}: CPU model, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_tile_d_follows_the_kernel_exponent_rule():
    op = torch.zeros(17, 4)
    op[0, 0], op[1, 1], op[2, 2], op[3, 3] = 8.0, 2.0 ** -37, float("inf"), float("nan")
    op[2, 0] = 1.0
    op[16, 1] = 3.0
    d = U.tile_d(op)
    assert d[0] == 0 and d[1] == 40 and d[2] == 3 and d[16] == 0      # Inf / NaN do not count; the third tile is its own group
    assert bool((d[4:16] == 0).all())                                 # all-zero rows, all-zero tile
    q = U.emulate_f16x2(op[:2].double())
    assert q[0, 0] == 8.0 and q[1, 1] == 0.0                          # 2^-40 of the tile maximum: flushed
