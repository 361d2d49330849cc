"""Sub-network search on the CPU (elastic_nn/search.py, search_ofa_net_sr.py): the arch space of S4 / X4 under both stage
indexings, canonical keys, MACs, the evolutionary search with a synthetic fitness, and the command line."""
import random

import pytest

from conftest import amd

KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])


@pytest.fixture(params=[True, False], ids=["compat", "intended"])
def compat(request):
    nets = amd("elastic_nn.networks")
    saved = (nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING)
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = request.param
    nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = request.param
    yield request.param
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = saved


_NETS = {}


def _net(kind):
    if kind not in _NETS:
        nets = amd("elastic_nn.networks")
        _NETS[kind] = (nets.OFAMobileNetS4 if kind == "s4" else nets.OFAMobileNetX4)(**KW)
    return _NETS[kind]


def _space(kind, compat_on):
    search = amd("elastic_nn.search")
    net = _net(kind)
    if kind == "s4":
        return search.ArchSpace(net, 4 if compat_on else 2)
    return search.ArchSpace(net)


def _check_valid(space, arch):
    assert space.valid(arch), arch
    assert len(arch["ks"]) == len(arch["e"]) == space.n_mb and len(arch["d"]) == space.n_stages
    if space.upscale is not None:
        assert space.upscale_of(arch) == space.upscale, arch
    space.apply(space.net, arch)
    space.net.get_active_net_config()    # the active path is well formed


@pytest.mark.parametrize("kind", ["s4", "x4"])
def test_sample_mutate_crossover_valid(kind, compat):
    space = _space(kind, compat)
    rng = random.Random(1)
    archs = [space.random_sample(rng) for _ in range(20)]
    for a in archs:
        _check_valid(space, a)
    for i in range(30):
        m = space.mutate(archs[i % 20], 0.3, rng)
        _check_valid(space, m)
        c = space.crossover(archs[i % 20], archs[(7 * i + 3) % 20], rng)
        _check_valid(space, c)
    assert space.mutate(archs[0], 0.0, rng) == archs[0]


def test_s4_upscale_fixed():
    search = amd("elastic_nn.search")
    nets = amd("elastic_nn.networks")
    saved = nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING
    try:
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = False
        for up in (2, 4):
            sp = search.ArchSpace(_net("s4"), up)
            rng = random.Random(up)
            assert all(sp.upscale_of(sp.random_sample(rng)) == up for _ in range(10))
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = True
        with pytest.raises(ValueError):     # quirk Q1: the shuffle stage reads a depth >= 2
            search.ArchSpace(_net("s4"), 2)
    finally:
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = saved


@pytest.mark.parametrize("kind", ["s4", "x4"])
def test_key_merges_inactive_blocks(kind, compat):
    space = _space(kind, compat)
    rng = random.Random(2)
    a = space.random_sample(rng)
    a["d"] = [space.d0_list[0]] + [min(space.d_list)] * (space.n_stages - 1)
    b = space.mutate(a, 0.0, rng)
    # the last block of every group is beyond the active depth when the depth is below the maximum
    for g in space.net.block_group_info:
        i = g[-1] - (2 if kind == "x4" else 0)
        if 0 <= i < space.n_mb:
            b["ks"][i] = 7 if a["ks"][i] != 7 else 3
    assert b != a and space.key(a) == space.key(b)
    c = dict(a, ks=list(a["ks"]))
    first = space.net.block_group_info[1 if kind == "x4" else 0][0] - (2 if kind == "x4" else 0)
    c["ks"][first] = 7 if a["ks"][first] != 7 else 3
    assert space.key(c) != space.key(a)


@pytest.mark.parametrize("kind", ["s4", "x4"])
def test_macs_equals_count_net_flops(kind, compat):
    search = amd("elastic_nn.search")
    pu = amd("imagenet_codebase.utils.pytorch_utils")
    space = _space(kind, compat)
    rng = random.Random(3)
    for _ in range(4):
        a = space.random_sample(rng)
        got = search.macs(space.net, a, (48, 40), space)
        space.net.set_active_subnet(ks=list(a["ks"]), e=list(a["e"]), d=list(a["d"]), pixel_d=a["pixel_d"])
        assert got == pu.count_net_flops(space.net, (1, 3, 48, 40)) > 0


def _synthetic_search(seed, budget_frac=0.6, pop=12, gens=5):
    search = amd("elastic_nn.search")
    space = _space("s4", True)
    rng = random.Random(99)
    costs = sorted(space.macs(space.net, space.random_sample(rng), (32, 32)) for _ in range(40))
    budget = costs[int(budget_frac * len(costs))] / 1e9
    calls = []

    def efficiency(a):
        return space.macs(space.net, a, (32, 32)) / 1e9

    def fitness(a):
        calls.append(space.key(a))
        return -efficiency(a) + 0.01 * sum(a["ks"]) + 0.02 * sum(a["e"])

    es = search.EvolutionSearch(space, fitness, efficiency, budget, population_size=pop, generations=gens, seed=seed,
                                mutate_prob=0.2)
    best, hist = es.run()
    return es, best, hist, calls, budget, efficiency


def test_evolution_search_synthetic_fitness():
    es, best, hist, calls, budget, eff = _synthetic_search(5)
    assert len(hist) == 6
    assert eff(best) <= budget
    for k in es.evaluated:
        assert es.costs[k] <= budget
    bests = [h["best_fitness"] for h in hist]
    assert all(b2 >= b1 for b1, b2 in zip(bests, bests[1:])), bests
    assert len(calls) == len(set(calls)) == len(es.evaluated)
    assert hist[-1]["best_fitness"] == es.cache[es.space.key(best)]


def test_evolution_search_deterministic():
    _, best1, h1, c1, _, _ = _synthetic_search(11)
    _, best2, h2, c2, _, _ = _synthetic_search(11)
    assert h1 == h2 and best1 == best2 and c1 == c2
    _, _, h3, c3, _, _ = _synthetic_search(12)
    assert c3 != c1


def test_cli_arguments():
    import search_ofa_net_sr as cli
    a = cli.parse_args(["--net", "x4", "--budget-ms", "2.5", "--lat-table", "t.json", "--calib-images", "8",
                        "--population", "4", "--generations", "2", "--seed", "3", "--synthetic", "--export", "out",
                        "--test-sizes", "64x64,48x80"])
    assert (a.net, a.budget_ms, a.budget_gmacs, a.lat_table, a.calib_images) == ("x4", 2.5, None, "t.json", 8)
    assert (a.population, a.generations, a.seed, a.synthetic, a.export) == (4, 2, 3, True, "out")
    assert a.test_sizes == [(64, 64), (48, 80)]
    b = cli.parse_args(["--budget-gmacs", "1.5", "--upscale", "2", "--checkpoint", "c.pth"])
    assert (b.net, b.budget_gmacs, b.upscale, b.checkpoint, b.export) == ("s4", 1.5, 2, "c.pth", None)
    with pytest.raises(SystemExit):
        cli.parse_args(["--budget-gmacs", "1", "--budget-ms", "1"])
    with pytest.raises(SystemExit):
        cli.parse_args([])
