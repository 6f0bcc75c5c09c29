"""GPU: the barostat kernels of csrc/gn_md.hip (gn_npt_*) against the fp64 emulation of tests/npt_util.py."""
import math

import numpy as np
import pytest
import torch

from tests import md_util as MU
from tests import npt_util as NU
from tests import pbc_util as U

pytestmark = pytest.mark.gpu

CUTOFF = 5.0
PAD = 4                                    # guard words on either side of every output
P0, BETA, TAU, DT, KT, MAX_STEP = 0.01, 5.0, 20.0, 0.5, 0.03, 0.05
CELLS = np.array([np.eye(3) * 5.0, U.ORTHO, np.array(U.TRICLINIC) * 2.08], dtype=np.float32)      # cubic, orthorhombic, triclinic
PRESSURES = np.array([0.05, -0.02, 0.013], dtype=np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from gotennet_amd._lib import call
    call(name, *args, _stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _padded(values, dtype=torch.float32, fill=-7):
    """-> (whole buffer, the view the kernel writes): ``values`` with PAD words of ``fill`` before and behind."""
    v = torch.as_tensor(np.asarray(values)).to(dtype).flatten()
    whole = torch.full((v.numel() + 2 * PAD,), fill, dtype=dtype)
    whole[PAD:PAD + v.numel()] = v
    whole = whole.cuda()
    return whole, whole[PAD:PAD + v.numel()]


def _pads_intact(whole, fill=-7):
    w = whole.cpu()
    return bool((w[:PAD] == fill).all()) and bool((w[-PAD:] == fill).all())


def _key(a=1234, b=0):
    return torch.tensor([a, b], dtype=torch.int64, device="cuda")


def _xi(key, step, n):
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    _call("gn_md_noise", _ptr(key), step, 2, n, _ptr(out))
    return out[:, 0].cpu().numpy().astype(np.float64)


def _volumes(cells):
    return NU.widths(cells)[1].astype(np.float32)


class Move:
    """One gn_npt_barostat call on padded buffers."""

    def __init__(self, cells, pressures, kT, key, step=7, stale=0, p0=P0, max_step=MAX_STEP, beta=BETA, tau=TAU, dt=DT):
        n = len(cells)
        self.n, self.cell0, self.vol = n, np.asarray(cells, dtype=np.float32), _volumes(cells)
        self.cell_w, self.cell = _padded(self.cell0)
        self.s_w, self.s = _padded(np.full(n, -3.0))
        self.inv_w, self.inv_s = _padded(np.full(n, -4.0))
        self.state_w, self.state = _padded([stale, step], torch.int32)
        self.reason_w, self.reason = _padded(np.zeros(n), torch.int32)
        vol, p = torch.tensor(self.vol).cuda(), torch.tensor(np.asarray(pressures, dtype=np.float32)).cuda()
        _call("gn_npt_barostat", _ptr(self.cell), _ptr(vol), _ptr(p), n, p0, beta, tau, dt, kT, max_step, _ptr(key), _ptr(self.s),
              _ptr(self.inv_s), _ptr(self.state), _ptr(self.reason))
        torch.cuda.synchronize()
        assert all(_pads_intact(w) for w in (self.cell_w, self.s_w, self.inv_w, self.state_w, self.reason_w))

    def untouched(self):
        return (np.array_equal(self.cell.cpu().numpy().reshape(-1, 3, 3), self.cell0) and bool((self.s == -3.0).all())
                and bool((self.inv_s == -4.0).all()))


def test_barostat_against_fp64():
    vol = _volumes(CELLS).astype(np.float64)
    assert 9.0 < vol[1] / vol[0] < 11.0 and 9.0 < vol[2] / vol[1] < 11.0            # volumes differ tenfold
    key, step = _key(77, 5), 7
    xi = _xi(key, step, 3)
    m = Move(CELLS, PRESSURES, KT, key, step)
    de = NU.delta_eps(PRESSURES, vol, P0, BETA, TAU, DT, KT, xi)
    assert bool((np.abs(de) < MAX_STEP).all())
    s, inv_s = m.s.cpu().numpy(), m.inv_s.cpu().numpy()
    assert bool((s != 1.0).all())
    us, ui = NU.ulps32(s, NU.scale(de)), NU.ulps32(inv_s, 1.0 / NU.scale(de))
    print(f"barostat: d_eps {de}, s {s}, ulps of s {us}, of 1/s {ui}")
    assert bool((us <= 1.0).all()) and bool((ui <= 1.0).all())
    assert np.array_equal(m.cell.cpu().numpy().reshape(3, 3, 3), CELLS * s.reshape(3, 1, 1))      # fp32 product, bit for bit
    assert m.state.tolist() == [0, step] and m.reason.tolist() == [0, 0, 0]
    # the noise is a function of (key, step): the same call repeats, another step or key does not
    assert np.array_equal(Move(CELLS, PRESSURES, KT, key, step).s.cpu().numpy(), s)
    for other in (Move(CELLS, PRESSURES, KT, key, step + 1), Move(CELLS, PRESSURES, KT, _key(78, 5), step), Move(CELLS, PRESSURES, KT, _key(77, 6), step)):
        assert not bool((other.s.cpu().numpy() == s).any())
    assert not np.array_equal(_xi(key, step + 1, 3), xi) and not np.array_equal(_xi(_key(78, 5), step, 3), xi)
    # kT = 0: the deterministic limit; the key is not read (a null pointer)
    d = Move(CELLS, PRESSURES, 0.0, None, step)
    de0 = NU.delta_eps(PRESSURES, vol, P0, BETA, TAU, DT, 0.0)
    s0 = d.s.cpu().numpy()
    assert bool((NU.ulps32(s0, NU.scale(de0)) <= 1.0).all()) and bool((NU.ulps32(d.inv_s.cpu().numpy(), 1.0 / NU.scale(de0)) <= 1.0).all())
    assert np.array_equal(d.cell.cpu().numpy().reshape(3, 3, 3), CELLS * s0.reshape(3, 1, 1))
    assert (s0[0] > 1.0) and (s0[1] < 1.0)                      # P_int above the target: the box grows; below: it shrinks


@pytest.mark.parametrize("bad", ["too_large", "too_small", "nan", "inf"])
def test_barostat_refuses_a_move_beyond_max_step(bad):
    p = PRESSURES.copy()
    # d_eps = -(BETA / TAU) (P0 - p) DT = +-2 * MAX_STEP for p = P0 +- 0.8
    p[1] = {"too_large": P0 + 0.8, "too_small": P0 - 0.8, "nan": float("nan"), "inf": float("inf")}[bad]
    if bad in ("too_large", "too_small"):
        assert abs(abs(float(NU.delta_eps(p[1], 1.0, P0, BETA, TAU, DT, 0.0))) - 2 * MAX_STEP) < 1e-6
    for kT, key in ((0.0, None), (KT, _key())):
        m = Move(CELLS, p, kT, key)
        assert m.state.tolist() == [1, 7] and m.reason.tolist() == [0, 2, 0]
        assert m.untouched()                                    # the refused box, and with it every other box of the call
    # exactly max_step is allowed (|d_eps| > max_step is the refusal)
    ok = Move(CELLS, PRESSURES, 0.0, None, max_step=float(np.abs(NU.delta_eps(PRESSURES, 1.0, P0, BETA, TAU, DT, 0.0)).max()) * (1 + 1e-12))
    assert ok.state.tolist() == [0, 7] and not ok.untouched()


@pytest.mark.parametrize("n_mol,step,log_len", [(3, 9, 4), (70, 0, 1), (130, 2 ** 20 + 3, 8)])
def test_pressure_against_fp64(n_mol, step, log_len):
    g = torch.Generator().manual_seed(n_mol)
    ke = torch.rand(n_mol, generator=g) * 3 + 0.1
    stress = torch.randn((n_mol, 3, 3), generator=g) * 0.01
    vol = torch.rand(n_mol, generator=g) * 2000 + 100
    p_w, p = _padded(np.full(n_mol, -3.0))
    log_w, log = _padded(np.full(log_len * n_mol * 2, -5.0))
    state = torch.tensor([0, step], dtype=torch.int32, device="cuda")
    dev = [t.cuda() for t in (ke, stress, vol)]
    _call("gn_npt_pressure", *(_ptr(t) for t in dev), n_mol, _ptr(p), _ptr(log), log_len, _ptr(state))
    torch.cuda.synchronize()
    ref = NU.pressure(ke.numpy(), stress.numpy(), vol.numpy())
    u = NU.ulps32(p.cpu().numpy(), ref)
    print(f"pressure n_mol={n_mol}: max ulps {u.max():.2f}")
    assert bool((u <= 2.0).all())
    assert _pads_intact(p_w) and _pads_intact(log_w) and state.tolist() == [0, step]
    rows = log.cpu().reshape(log_len, n_mol, 2)
    k = step % log_len
    assert torch.equal(rows[k, :, 0], vol) and torch.equal(rows[k, :, 1], p.cpu())
    assert bool((rows[[r for r in range(log_len) if r != k]] == -5.0).all())


def test_rescale_is_the_fp32_product():
    batch = MU.batch_vector()                                   # 2 + 5 + 9 atoms: molecule boundaries inside a wave
    N = batch.shape[0]
    assert N == 16
    g = torch.Generator().manual_seed(4)
    pos, vel = torch.randn((N, 3), generator=g) * 7, torch.randn((N, 3), generator=g)
    s = np.array([1.0012345, 0.9987654, 1.0000001], dtype=np.float32)
    inv_s = (1.0 / s.astype(np.float64)).astype(np.float32)
    pos_w, pos_d = _padded(pos.numpy())
    vel_w, vel_d = _padded(vel.numpy())
    state = torch.tensor([0, 3], dtype=torch.int32, device="cuda")
    dev = [batch.cuda(), torch.tensor(s).cuda(), torch.tensor(inv_s).cuda()]
    _call("gn_npt_rescale", _ptr(pos_d), _ptr(vel_d), *(_ptr(t) for t in dev), N, 3, _ptr(state))
    torch.cuda.synchronize()
    b = batch.numpy()
    assert np.array_equal(pos_d.cpu().numpy().reshape(N, 3), pos.numpy() * s[b][:, None])
    assert np.array_equal(vel_d.cpu().numpy().reshape(N, 3), vel.numpy() * inv_s[b][:, None])
    assert not np.array_equal(pos_d.cpu().numpy().reshape(N, 3), pos.numpy())
    assert _pads_intact(pos_w) and _pads_intact(vel_w)


def _guard(cells, ranges=None, stale=0):
    n = len(cells)
    state_w, state = _padded([stale, 5], torch.int32)
    reason_w, reason = _padded(np.zeros(n), torch.int32)
    r = None if ranges is None else torch.tensor(ranges, dtype=torch.int32).reshape(n, 3).cuda()
    c = torch.tensor(np.asarray(cells, dtype=np.float32)).cuda()
    _call("gn_npt_cell_guard", _ptr(c), n, CUTOFF, _ptr(r), _ptr(state), _ptr(reason))
    torch.cuda.synchronize()
    assert _pads_intact(state_w) and _pads_intact(reason_w)
    return state.tolist(), reason.tolist()


def test_cell_guard():
    below = float(np.nextafter(np.float32(10.0), np.float32(0)))
    cube, narrow_cube = np.eye(3) * 10.0, np.eye(3) * below
    skew = np.array([[10.5, 0, 0], [8.0, 8.0, 0], [0, 0, 12.0]])           # every lattice vector longer than 10, one width 7.4
    w, _ = NU.widths(skew)
    assert np.linalg.norm(skew, axis=1).min() > 2 * CUTOFF and w.min() < 2 * CUTOFF - 1.0
    flat = np.array([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]])             # coplanar rows: no volume
    assert NU.widths(flat)[1][0] == 0.0
    # the minimum-image rule: w_k >= 2 * cutoff
    assert _guard([cube, np.array(U.TRICLINIC), np.array(U.ORTHO)]) == ([0, 5], [0, 0, 0])
    assert _guard([cube, narrow_cube, skew, cube, flat]) == ([1, 5], [0, 1, 1, 0, 1])
    assert _guard([narrow_cube]) == ([1, 5], [1]) and _guard([np.diag([12.0, 12.0, below])]) == ([1, 5], [1])
    # against stored image ranges: floor(cutoff / w + 1/2 + 2^-6) <= R
    four = np.eye(3) * 4.0
    assert math.floor(CUTOFF / 4.0 + 0.5 + 2.0 ** -6) == 1
    assert _guard([four], [[1, 1, 1]]) == ([0, 5], [0])
    assert _guard([four], [[0, 0, 0]]) == ([1, 5], [1])
    wide = np.eye(3) * 12.0                                               # floor(5 / 12 + 1/2 + 1/64) = 0
    assert _guard([four, four, wide, flat, four], [[1, 1, 1], [1, 0, 1], [0, 0, 0], [3, 3, 3], [3, 3, 3]]) == ([1, 5], [0, 1, 0, 1, 0])
    assert _guard([cube], [[0, 0, 0]]) == ([1, 5], [1])                    # width 10: 1/2 + 1/2 + 1/64 needs R = 1
    assert _guard([np.full((3, 3), float("nan"))], [[3, 3, 3]]) == ([1, 5], [1]) and _guard([np.full((3, 3), float("inf"))]) == ([1, 5], [1])


def test_a_set_flag_freezes_every_npt_kernel():
    # the barostat: a move that would act, and one that would be refused
    for p in (PRESSURES, np.array([0.05, 5.0, float("nan")], dtype=np.float32)):
        m = Move(CELLS, p, KT, _key(), stale=1)
        assert m.untouched() and m.state.tolist() == [1, 7] and m.reason.tolist() == [0, 0, 0]
    # the pressure and its ring row
    n = 3
    p_w, p = _padded(np.full(n, -3.0))
    log_w, log = _padded(np.full(4 * n * 2, -5.0))
    state_w, state = _padded([1, 9], torch.int32)
    ke, stress, vol = torch.ones(n).cuda(), torch.ones((n, 3, 3)).cuda(), torch.full((n,), 100.0).cuda()
    _call("gn_npt_pressure", _ptr(ke), _ptr(stress), _ptr(vol), n, _ptr(p), _ptr(log), 4, _ptr(state))
    # the rescale
    pos_w, pos = _padded(np.full(16 * 3, 2.0))
    vel_w, vel = _padded(np.full(16 * 3, 3.0))
    s, batch = torch.full((3,), 1.5).cuda(), MU.batch_vector().cuda()
    _call("gn_npt_rescale", _ptr(pos), _ptr(vel), _ptr(batch), _ptr(s), _ptr(s), 16, 3, _ptr(state))
    torch.cuda.synchronize()
    for whole, view, fill in ((p_w, p, -3.0), (log_w, log, -5.0), (pos_w, pos, 2.0), (vel_w, vel, 3.0)):
        assert _pads_intact(whole) and bool((view == fill).all())
    assert _pads_intact(state_w) and state.tolist() == [1, 9]
    # the guard: cells that would fire
    assert _guard([np.eye(3) * 4.0, np.zeros((3, 3))], stale=1) == ([1, 5], [0, 0])
    assert _guard([np.eye(3) * 4.0], [[0, 0, 0]], stale=1) == ([1, 5], [0])
    # the same calls with the flag clear do act: the assertions above are not vacuous
    state = torch.tensor([0, 9], dtype=torch.int32, device="cuda")
    _call("gn_npt_pressure", _ptr(ke), _ptr(stress), _ptr(vol), n, _ptr(p), _ptr(log), 4, _ptr(state))
    _call("gn_npt_rescale", _ptr(pos), _ptr(vel), _ptr(batch), _ptr(s), _ptr(s), 16, 3, _ptr(state))
    torch.cuda.synchronize()
    assert bool((p != -3.0).all()) and bool((pos == 3.0).all()) and bool((vel == 4.5).all())
    assert bool((log.reshape(4, n, 2)[1] != -5.0).all()) and bool((log.reshape(4, n, 2)[[0, 2, 3]] == -5.0).all())


def test_noise_scale():
    """4096 boxes of one volume at P_int = P0: d_eps = 3 ln s is the noise term alone, mean 0 and variance
    2 kT beta dt / (V tau).  The keys are fixed, so the sample is."""
    n, vol, kT, beta, dt, tau = 4096, 1000.0, 0.02, 5.0, 0.5, 50.0
    q = kT * beta * dt / (vol * tau)
    sigma = math.sqrt(2 * q)
    assert 0.5e-6 <= q <= 2e-6
    # the fp32 rounding of s (2^-24 relative, three times that on d_eps) sits below the statistical bounds
    assert 3 * 2.0 ** -24 < 5 * sigma / math.sqrt(n) and (3 * 2.0 ** -24) ** 2 < 0.01 * 5 * math.sqrt(2 / (n - 1)) * sigma ** 2
    cells = np.broadcast_to(np.eye(3, dtype=np.float32) * 10.0, (n, 3, 3)).copy()
    m = Move(cells, np.full(n, 0.25, dtype=np.float32), kT, _key(20240607, 3), step=11, p0=0.25, beta=beta, tau=tau, dt=dt)
    assert m.state.tolist() == [0, 11] and not bool(m.reason.any())
    de = 3.0 * np.log(m.s.cpu().numpy().astype(np.float64))
    mean, var = float(de.mean()), float(de.var(ddof=1))
    print(f"noise scale: n = {n}, mean {mean:.3e} (bound {5 * sigma / math.sqrt(n):.3e}), variance / expected - 1 = "
          f"{var / sigma ** 2 - 1:.3e} (bound {5 * math.sqrt(2 / (n - 1)):.3e})")
    assert abs(mean) <= 5 * sigma / math.sqrt(n)
    assert abs(var / sigma ** 2 - 1) <= 5 * math.sqrt(2 / (n - 1))
    # and it is the documented noise: gn_md_noise(key, step, 2, n)[:, 0], box by box
    xi = _xi(_key(20240607, 3), 11, n)
    assert bool((NU.ulps32(m.s.cpu().numpy(), NU.scale(sigma * xi)) <= 1.0).all())
    assert np.array_equal(m.cell.cpu().numpy().reshape(n, 3, 3), cells * m.s.cpu().numpy().reshape(n, 1, 1))
