"""Sub-network extraction (CPU): OFAMobileNetS4 / OFAMobileNetX4.get_active_net_config() / get_active_subnet() and the
static networks they describe (imagenet_codebase/networks/sr_static.py): JSON round trips, structure against the
supernet's active path under both stage indexings (COMPAT_REFERENCE_INDEXING), state-dict spelling, and
the way back into a supernet (load_weights_from_net).  Weight-preserving extraction runs the kernel transform on the GPU
and is covered by test_hip_specialize.py."""
import json
import random

import pytest
import torch

from conftest import amd

S4_KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
X4_KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])

# (kind, setting): a fixed set_active_subnet call or a seeded sample_active_subnet
SETTINGS = [("set", dict(ks=7, e=6, d=4, pixel_d=2)), ("set", dict(ks=3, e=3, d=2, pixel_d=1)),
            ("set", dict(ks=5, e=4, d=3, pixel_d=2)), ("sample", 0), ("sample", 1), ("sample", 7)]


@pytest.fixture(params=[True, False], ids=["compat", "intended"])
def compat(request):
    nets = amd("elastic_nn.networks")
    saved = (nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING)
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = request.param
    nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = request.param
    yield request.param
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = saved


def _supernet(kind, transform=True):
    nets = amd("elastic_nn.networks")
    dop = amd("elastic_nn.modules.dynamic_op")
    saved = dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1 if transform else None
    try:
        return nets.OFAMobileNetS4(**S4_KW) if kind == "s4" else nets.OFAMobileNetX4(**X4_KW)
    finally:
        dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = saved


def _apply(net, setting):
    kind, arg = setting
    if kind == "set":
        net.set_active_subnet(**{k: (list(v) if isinstance(v, list) else v) for k, v in arg.items()})
    else:
        random.seed(arg)
        net.sample_active_subnet()


def _active_mb(net):
    """(in_channels, K, mid) of every active MB block of the supernet, in execution order"""
    out = []
    if hasattr(net, "_depth_of"):   # X4
        for g in range(1, 9):
            for idx in net.block_group_info[g][:net._depth_of(g)]:
                m = net.blocks[idx].mobile_inverted_conv
                out.append((64, m.active_kernel_size, m.active_middle_channel(64)))
        return out
    for kind, m in net.active_block_sequence():
        if kind == "mb":
            out.append((64, m.active_kernel_size, m.active_middle_channel(64)))
    return out


@pytest.mark.parametrize("kind", ["s4", "x4"])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "%s%s" % (s[0], s[1] if s[0] == "sample" else
                                                                         "_k%(ks)d_e%(e)d_d%(d)d_pd%(pixel_d)d" % s[1]))
def test_active_net_config(kind, setting, compat):
    st = amd("imagenet_codebase.networks.sr_static")
    net = _supernet(kind)
    _apply(net, setting)
    cfg = net.get_active_net_config()
    assert json.loads(json.dumps(cfg)) == cfg
    static = st.build_static_net(cfg)
    assert static.config == cfg
    assert type(static).__name__ == ("SRNetS4" if kind == "s4" else "SRNetX4")

    mbs = [b for b in cfg["blocks"] if b["name"] == "MobileInvertedResidualBlock"]
    want = _active_mb(net)
    assert len(mbs) == len(want) == len(static.mb_blocks())
    got = [(b["mobile_inverted_conv"]["in_channels"], b["mobile_inverted_conv"]["kernel_size"],
            b["mobile_inverted_conv"]["mid_channels"]) for b in mbs]
    assert got == want
    for b, sb in zip(mbs, static.mb_blocks()):
        mb = sb.mobile_inverted_conv
        assert mb.depth_conv.conv.weight.shape[0] == b["mobile_inverted_conv"]["mid_channels"]
        assert mb.depth_conv.conv.kernel_size == (b["mobile_inverted_conv"]["kernel_size"],) * 2
    if kind == "s4":
        assert cfg["upscale"] == net.active_upscale()
        assert cfg["n_mb"] == len(want)
        n_shuffle = len(cfg["blocks"]) - cfg["n_mb"]
        assert 2 ** n_shuffle == net.active_upscale()
    else:
        assert cfg["upscale"] == 1     # the X4 autoencoder: as many shuffle as unshuffle blocks
        assert cfg["n_enc"] + cfg["n_dec"] == len(want)
    assert cfg["bn"] == net.get_bn_param()


def test_upscale_follows_the_indexing_quirk():
    """compat indexing: the shuffle stage reads runtime_depth[0] (Q1), so pixel_d=1 still gives a 4x network at d=2"""
    nets = amd("elastic_nn.networks")
    saved = nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING
    try:
        for c, up in ((True, 4), (False, 2)):
            nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = c
            net = _supernet("s4")
            net.set_active_subnet(ks=3, e=3, d=2, pixel_d=1)
            assert net.get_active_net_config()["upscale"] == up == net.active_upscale()
    finally:
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = saved


def _structure(m):
    return [(k, tuple(v.shape), v.dtype) for k, v in m.state_dict().items()]


@pytest.mark.parametrize("kind", ["s4", "x4"])
@pytest.mark.parametrize("setting", SETTINGS[:4], ids=lambda s: str(s[1]))
def test_subnet_without_weights_matches_config(kind, setting, compat):
    st = amd("imagenet_codebase.networks.sr_static")
    net = _supernet(kind)
    _apply(net, setting)
    sub = net.get_active_subnet(preserve_weight=False)
    ref = st.build_static_net(net.get_active_net_config())
    assert _structure(sub) == _structure(ref)
    assert sub.config == ref.config
    assert [type(m).__name__ for m in sub.modules()] == [type(m).__name__ for m in ref.modules()]


def test_static_state_dict_spelling():
    net = _supernet("s4")
    net.set_active_subnet(ks=[3, 5, 7, 3] * 4, e=[3, 4, 6, 4] * 4, d=3, pixel_d=2)
    sub = net.get_active_subnet(preserve_weight=False)
    sd = sub.state_dict()
    cfg = net.get_active_net_config()
    n_mb = cfg["n_mb"]
    for i, b in enumerate(cfg["blocks"][:n_mb]):
        p = "blocks.%d.mobile_inverted_conv." % i
        mid, K = b["mobile_inverted_conv"]["mid_channels"], b["mobile_inverted_conv"]["kernel_size"]
        assert tuple(sd[p + "inverted_bottleneck.conv.weight"].shape) == (mid, 64, 1, 1)
        assert tuple(sd[p + "depth_conv.conv.weight"].shape) == (mid, 1, K, K)
        assert tuple(sd[p + "point_linear.conv.weight"].shape) == (64, mid, 1, 1)
        for part, c in (("inverted_bottleneck", mid), ("depth_conv", mid), ("point_linear", 64)):
            for t in ("weight", "bias", "running_mean", "running_var"):
                assert tuple(sd[p + part + ".bn." + t].shape) == (c,)
            assert p + part + ".bn.num_batches_tracked" in sd
    for i in range(n_mb, len(cfg["blocks"])):
        assert tuple(sd["blocks.%d.conv.weight" % i].shape) == (256, 64, 5, 5)
    # blocks numbered consecutively, no supernet spelling, no transform matrices
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("blocks.")})
    assert idx == list(range(len(cfg["blocks"])))
    assert not any(".conv.conv." in k or ".bn.bn." in k or "_matrix" in k for k in sd)


def test_static_checkpoint_maps_back_into_a_supernet(compat):
    _maps_back("s4", compat)


def test_static_checkpoint_maps_back_into_a_supernet_x4():
    """(X4 under the compat indexing never activates all blocks: its first encoder / decoder stages read the clipped
    shuffle depth, Q2 -- so the full static net exists only under the intended indexing)"""
    nets = amd("elastic_nn.networks")
    saved = nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING
    nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = False
    try:
        _maps_back("x4", False)
    finally:
        nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = saved


def _maps_back(kind, compat):
    """the static net of the full supernet (every block active, largest kernel / width) is loaded into a fresh supernet
    through load_weights_from_net: every static tensor lands on its supernet counterpart"""
    net = _supernet(kind)
    if kind == "s4":
        net.set_active_subnet(ks=7, e=6, d=4, pixel_d=4 if compat else 2)   # compat: pixel_d lands on MB stage 4 (Q2)
        assert net.get_active_net_config()["n_mb"] == 16
    else:
        net.set_active_subnet(ks=7, e=6, d=4, pixel_d=2)
        assert net.get_active_net_config()["n_enc"] == 16
    sub = net.get_active_subnet(preserve_weight=False)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for t in sub.state_dict().values():
            if t.is_floating_point():
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    sd = sub.state_dict()
    fresh = _supernet(kind)
    fresh.load_weights_from_net(sd)
    own = fresh.state_dict()
    for k, v in sd.items():
        sk = k.replace(".bn.", ".bn.bn.") if ".mobile_inverted_conv." in k else k
        if ".mobile_inverted_conv." in k and k.endswith("conv.weight"):
            sk = k[:-len("conv.weight")] + "conv.conv.weight"
        assert torch.equal(own[sk], v), k


def test_static_net_refuses_cpu_tensors():
    """the static forward has no CPU / ATen path for its MB blocks"""
    C = amd("_C")
    net = _supernet("s4")
    net.set_active_subnet(ks=3, e=3, d=2, pixel_d=1)
    sub = net.get_active_subnet(preserve_weight=False).eval()
    st = amd("imagenet_codebase.networks.sr_static")
    with pytest.raises(C.OfasrError):
        with torch.no_grad():
            st.run_mb_blocks(torch.zeros(1, 64, 4, 4), list(sub.mb_blocks()))
