"""CPU: the host side of parameter gradients -- which configurations are accepted, and the pack <-> parameter layout."""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN_DIR, load_case

ACCEPTED = ["l1_nosep_scale_f32", "l2_sep_f32", "l3_sep_scale_f32", "l4_sep_f32", "l5_sep_f32", "l6_nosep_scale_f32",
            "l7_mixed_jointhtr_gated", "l8_sep_tln_f32", "l2_mixed_f64ch", "opt_act_ssp", "opt_act_mish_l4",
            "opt_act_norej_joint", "opt_act_tanh_l3_gated", "opt_aggr_max_l3", "opt_aggr_mean_l2", "opt_aggr_mean_l5_nosep",
            "opt_bessel_norej", "opt_gauss_jointhtr_gated", "opt_jointhtr_l3_tanh", "opt_layernorm_tln", "opt_noupd_act",
            "opt_tln_l4"]
FULL = ["c1_qm9_small_seeded", "c2_model_3mol_seeded", "c2_model_lmax4_1mol_seeded"]
REJECTED = ["opt_act_gelu_mlpa_linwa", "opt_evec16_emlp48", "opt_linw_act_l3", "opt_mlp_linwa_ln_gated",
            "opt_mlpa_linw_postln"]


def _net(cfg):
    import gotennet_amd
    keys = ("n_atom_basis", "n_interactions", "n_rbf", "lmax", "num_heads", "scale_edge", "sep_dir", "sep_tensor", "max_z",
            "radial_basis", "edge_updates", "sep_htr", "layernorm", "steerable_norm", "activation", "aggr", "evec_dim",
            "emlp_dim", "edge_ln")
    return gotennet_amd.GotenNet(cutoff_fn=gotennet_amd.CosineCutoff(cfg.get("cutoff", 5.0)),
                                 **{k: cfg[k] for k in keys if k in cfg})


def test_every_fixture_is_classified_by_the_support_check():
    """Every golden fixture is accepted exactly when it has no composed edge update (its width is a power of two), and the
    accepted fixtures that carry a head are ACCEPTED, the list the GPU parity test runs (the full-size seeded ones, FULL,
    carry no weights and run on their own)."""
    from gotennet_amd import engine
    from tests.golden_util import case_names
    accepted = []
    for name in case_names():
        cfg = load_case(name)[0]
        parts = str(cfg.get("edge_updates", "")).split("_")
        composed = any(p in ("mlp", "mlpa", "linw", "linwa") for p in parts)
        try:
            engine.check_param_grads_supported(_net(cfg).config())
            ok = True
        except NotImplementedError:
            ok = False
        assert ok != composed, name
        if ok and "head/out_net.1.out_net.0.weight" in np.load(os.path.join(GOLDEN_DIR, name + ".npz")).files:
            accepted.append(name)
    assert sorted(accepted) == sorted(ACCEPTED)
    assert sorted(set(case_names()) - set(accepted)) == sorted(REJECTED + FULL + ["l2_sep_shuffled_noloop"])


@pytest.mark.parametrize("name", ACCEPTED + FULL + ["c2_full_forward_seeded"])
def test_supported_configurations_are_accepted(name):
    from gotennet_amd import engine
    cfg = load_case(name)[0]
    engine.check_param_grads_supported(_net(cfg).config())


@pytest.mark.parametrize("name", REJECTED)
def test_composed_edge_updates_are_rejected(name):
    from gotennet_amd import engine
    cfg = load_case(name)[0]
    with pytest.raises(NotImplementedError, match="composed edge updates"):
        engine.check_param_grads_supported(_net(cfg).config())


def test_embedded_width_is_rejected():
    import gotennet_amd
    from gotennet_amd import engine
    net = gotennet_amd.GotenNet(n_atom_basis=96, n_interactions=2, n_rbf=8, lmax=2, num_heads=8,
                                cutoff_fn=gotennet_amd.CosineCutoff(5.0))
    with pytest.raises(NotImplementedError, match="power of two"):
        engine.check_param_grads_supported(net.config())


@pytest.mark.parametrize("kw", [dict(lmax=1), dict(lmax=2, sep_dir=True, sep_tensor=True), dict(lmax=5),
                                dict(lmax=2, sep_htr=False), dict(lmax=2, edge_updates=False), dict(lmax=2, layernorm="layer"),
                                dict(lmax=3, n_interactions=3, sep_dir=True, edge_updates="gated")])
def test_unpack_is_the_inverse_of_the_pack(kw):
    import gotennet_amd
    from gotennet_amd.gotennet import unpack_param_grads
    kw = dict(dict(n_atom_basis=32, n_interactions=2, n_rbf=8, num_heads=4, max_z=10), **kw)
    torch.manual_seed(0)
    net = gotennet_amd.GotenNet(cutoff_fn=gotennet_amd.CosineCutoff(5.0), **kw)
    with torch.no_grad():
        for p in net.parameters():
            p.uniform_(-1, 1)
    out = unpack_param_grads(net, net.packed_weights())
    named = dict(net.named_parameters())
    assert list(out) == list(named)
    for n, p in named.items():
        assert out[n].shape == p.shape, n
        assert torch.equal(out[n], p.detach()), n


def test_parameter_grads_is_off_by_default():
    import gotennet_amd
    from gotennet_amd.outputs import Atomwise, AtomwiseV3
    kw = dict(n_atom_basis=32, n_interactions=1, n_rbf=8, lmax=1, num_heads=4, cutoff_fn=gotennet_amd.CosineCutoff(5.0))
    assert gotennet_amd.GotenNet(**kw).parameter_grads is False
    assert gotennet_amd.GotenNetWrapper(**kw).parameter_grads is False
    assert Atomwise(n_in=32).parameter_grads is False
    assert AtomwiseV3(n_in=32).parameter_grads is False
