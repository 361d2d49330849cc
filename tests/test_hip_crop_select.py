"""ofasr_aug_select (csrc/augment.hip) and the best-of-K resident loader on the GPU against the host statement
(augment.aug_select_np, itself pinned to the plain statement and to routing.py by tests/test_crop_select.py): choice, all
K activities and the output table bit for bit, and the batches of every provider those of the existing gather for the
winners the host statement names."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd
from test_video_pair import PAIRS, make_pair_pools, write_video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB_SHAPES = [(40, 56), (33, 47), (16, 16)]
YUV_SHAPES = [(38, 54), (64, 48)]
BIG = (140, 150)                      # holds the smallest crop of two row strips, S = 129
ANGLES = [0.0, 90.0, -33.3, 45.0, 180.0, 17.25]


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _textured(rng, h, w, ch):
    """noise whose amplitude changes from block to block, so crops differ in activity, with one flat block"""
    amp = rng.randint(0, 128, (-(-h // 8), -(-w // 8)))
    amp[0, 0] = 0
    amp = np.kron(amp, np.ones((8, 8), np.int64))[:h, :w]
    shape = (h, w, ch) if ch else (h, w)
    noise = rng.randint(-128, 128, shape)
    return np.clip(128 + noise * (amp[..., None] if ch else amp) // 128, 0, 255).astype(np.uint8)


def _frame(rng, h, w):
    return (_textured(rng, h, w, 0), rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8),
            rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8))


def _on_device(host, lead):
    """the pool on the device, `lead` bytes past an aligned address: lead = 0 serves the wide loads, 1 the byte loads"""
    buf = torch.empty(host.size + lead, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    dev = buf[lead:]
    dev.copy_(torch.from_numpy(host))
    return dev


@pytest.fixture(scope="module")
def rgb():
    rng = np.random.RandomState(21)
    imgs = [_textured(rng, h, w, 3) for (h, w) in RGB_SHAPES + [BIG]]
    order = [3, 0, 1, 2]               # the 16 x 16 image last: its crop ends on the pool's last byte
    host = np.concatenate([imgs[k].reshape(-1) for k in order])
    offs = {k: int(sum(imgs[j].size for j in order[:order.index(k)])) for k in order}
    return {"imgs": imgs, "offs": offs, "host": host, "dev": {lead: _on_device(host, lead) for lead in (0, 1)}}


@pytest.fixture(scope="module")
def yuv():
    rng = np.random.RandomState(22)
    frames = [_frame(rng, h, w) for (h, w) in YUV_SHAPES + [BIG]]
    host = np.concatenate([p.reshape(-1) for f in frames for p in f])
    offs = [int(o) for o in np.cumsum([0] + [f[0].size * 3 // 2 for f in frames])[:-1]]
    return {"frames": frames, "offs": offs, "host": host, "dev": {lead: _on_device(host, lead) for lead in (0, 1)}}


def _corners(h, w, S, rng):
    """(0, 0), the right and bottom edges, odd corners, and drawn ones, inside the image"""
    fixed = [(0, 0), (h - S, w - S), (0, w - S), (h - S, 0), (min(1, h - S), min(3, w - S)), (min(5, h - S), min(7, w - S))]
    return fixed + [(int(rng.randint(0, h - S + 1)), int(rng.randint(0, w - S + 1))) for _ in range(4)]


def _samples(shapes, S, K, seed):
    """[(image, [K parameter sets])]: every image that holds the crop, its corners dealt round the K candidates"""
    rng = np.random.RandomState(seed)
    out = []
    for k, (h, w) in enumerate(shapes):
        if min(h, w) < S:
            continue
        cs = _corners(h, w, S, rng)
        ps = [(i, j, bool(rng.randint(2)), ANGLES[rng.randint(len(ANGLES))]) for (i, j) in cs]
        n = -(-len(ps) // K)
        for s in range(n):
            out.append((k, [ps[(s * K + c) % len(ps)] for c in range(K)]))
    return out


def _check(got, want):
    table, choice, act = got
    w_choice, w_act, w_table = want
    assert choice.dtype == torch.int32 and act.dtype == torch.int64 and table.dtype == torch.int64
    assert np.array_equal(act.cpu().numpy(), w_act), "activities differ"
    assert np.array_equal(choice.cpu().numpy(), w_choice), "choices differ"
    assert np.array_equal(table.cpu().numpy(), w_table), "tables differ"


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("S", [16, 15])
def test_rgb_pool_equals_the_host_statement(rgb, S, K, lead):
    aug, ops = _aug(), amd("ops")
    samples = _samples(RGB_SHAPES, S, K, 100 * S + K)
    assert {k for k, _ in samples} == {0, 1, 2}        # at S = 16 the crop of the 16 x 16 image is the image
    table = aug.make_table([(rgb["offs"][k],) + RGB_SHAPES[k] + (p,) for k, ps in samples for p in ps], S)
    got = ops.aug_select(rgb["dev"][lead], table.to(DEV), len(samples), K, S)
    want = aug.aug_select_np(rgb["host"], table.numpy(), len(samples), K, S, aug.LAYOUT_RGB)
    _check(got, want)
    choice, act = aug.select_candidates_np([rgb["imgs"][k] for k, _ in samples], [ps for _, ps in samples], S)
    assert np.array_equal(want[0], choice) and np.array_equal(want[1], act)        # ... and the plain statement
    if K > 1:
        assert len(set(want[0].tolist())) > 1                                      # the cases do exercise the choice


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("S", [16, 18])
def test_yuv420_pool_equals_the_host_statement(yuv, S, K, lead):
    aug, ops = _aug(), amd("ops")
    samples = _samples(YUV_SHAPES, S, K, 200 * S + K)
    table = aug.make_table([(yuv["offs"][k],) + YUV_SHAPES[k] + (p,) for k, ps in samples for p in ps], S, yuv420=True)
    got = ops.aug_select(yuv["dev"][lead], table.to(DEV), len(samples), K, S, yuv420=True)
    want = aug.aug_select_np(yuv["host"], table.numpy(), len(samples), K, S, aug.LAYOUT_YUV420)
    _check(got, want)
    choice, act = aug.select_candidates_np([yuv["frames"][k][0] for k, _ in samples], [ps for _, ps in samples], S)
    assert np.array_equal(want[0], choice) and np.array_equal(want[1], act)


@pytest.mark.parametrize("f", [2, 4])
def test_paired_pool_copies_both_blocks_of_the_winner(f):
    aug, ops = _aug(), amd("ops")
    S, K = 16, 3
    pools = make_pair_pools(f)
    rng = np.random.RandomState(f)
    samples = []
    for k, (_, (h, w)) in enumerate(PAIRS[f]):
        for _ in range(3):
            samples.append((k, [(int(rng.randint(0, h - S // f + 1)), int(rng.randint(0, w - S // f + 1)),
                                 bool(rng.randint(2)), ANGLES[rng.randint(len(ANGLES))]) for _ in range(K)]))
    samples.append((0, [(0, 0, False, 0.0), (PAIRS[f][0][1][0] - S // f, PAIRS[f][0][1][1] - S // f, True, 90.0), (1, 1, False, 45.0)]))
    rows = [(pools["hr_offs"][k],) + PAIRS[f][k][0] + (pools["lr_offs"][k],) + PAIRS[f][k][1] + (p,)
            for k, ps in samples for p in ps]
    table = aug.make_pair_table(rows, S, f)
    n = len(samples)
    hr_dev, lr_dev = torch.from_numpy(pools["hr_host"]).to(DEV), torch.from_numpy(pools["lr_host"]).to(DEV)
    got = ops.aug_select(hr_dev, table.to(DEV), n, K, S, yuv420=True, blocks=2)
    want = aug.aug_select_np(pools["hr_host"], table.numpy(), n, K, S, aug.LAYOUT_YUV420)
    _check(got, want)
    assert want[2].shape == (2, n, 12)
    choice, act = aug.select_candidates_np([pools["hr"][k][0] for k, _ in samples],
                                           [[aug.pair_hr_params(p, f) for p in ps] for _, ps in samples], S)
    assert np.array_equal(want[0], choice) and np.array_equal(want[1], act)
    winners = [(pools["hr_offs"][k],) + PAIRS[f][k][0] + (pools["lr_offs"][k],) + PAIRS[f][k][1] + (ps[c],)
               for (k, ps), c in zip(samples, choice)]
    assert np.array_equal(want[2], aug.make_pair_table(winners, S, f).numpy())
    # the table goes to the pair gather as it is
    hr, lr = ops.aug_gather_yuv420_pair(hr_dev, lr_dev, got[0], n, S, f)
    ref_hr, ref_lr = aug.gather_yuv420_pair_np(pools["hr_host"], pools["lr_host"], want[2], S, f,
                                               amd("video").yuv_coeffs("bt601", False)[0])
    assert np.array_equal(hr.cpu().numpy(), ref_hr) and np.array_equal(lr.cpu().numpy(), ref_lr)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("layout", ["rgb", "yuv420"])
def test_two_row_strips(rgb, yuv, layout, lead):
    """S = 129 is the smallest crop the first launch cuts into two strips: the vertical differences across the seam"""
    aug, ops = _aug(), amd("ops")
    S, K = 129, 2
    assert aug.aug_select_strips(S - 1) == 1 and aug.aug_select_strips(S) == 2
    src = rgb if layout == "rgb" else yuv
    k = 3 if layout == "rgb" else 2
    h, w = BIG
    cands = [[(0, 0, False, 0.0), (11, 21, True, 30.0)], [(h - S, w - S, False, 0.0), (h - S, 0, False, 0.0)],
             [(3, w - S, True, -45.0), (10, 20, False, 0.0)]]
    table = aug.make_table([(src["offs"][k], h, w, p) for ps in cands for p in ps], S, yuv420=layout != "rgb")
    got = ops.aug_select(src["dev"][lead], table.to(DEV), len(cands), K, S, yuv420=layout != "rgb")
    _check(got, aug.aug_select_np(src["host"], table.numpy(), len(cands), K, S, layout))
    img = rgb["imgs"][3] if layout == "rgb" else yuv["frames"][2][0]
    assert np.array_equal(got[2].cpu().numpy(), aug.select_candidates_np([img] * 3, cands, S)[1])


@pytest.mark.parametrize("layout", ["rgb", "yuv420"])
def test_out_of_contract_rows_are_clamped(rgb, yuv, layout):
    """values only, as the gathers' clamp tests: what the clamped rows give, and the call returns OFASR_OK"""
    aug, ops = _aug(), amd("ops")
    src, S, K = (rgb if layout == "rgb" else yuv), 16, 4
    nb = src["host"].size
    off = src["offs"][1]
    ident = tuple(aug.rotate_coeffs(0.0, S))
    rows = []
    for (i, j, o, H, W) in ((-5, 10 ** 6, off, 33, 47), (10 ** 9, -1, off, 33, 47), (3, 4, -17, 40, 56), (0, 0, nb + 99, 40, 56),
                            (2, 60, nb - 1000, 40, 96), (7, 3, off + 8, 1 << 40, 1 << 40), (-2 ** 40, 2 ** 40, 2 ** 50, 5, 5),
                            (1, 1, nb - 700, 16, 1 << 30)):
        rows.append((o, H, W, i, j, 0) + ident)
    table = torch.tensor(rows, dtype=torch.int64)
    for lead in (0, 1):
        got = ops.aug_select(src["dev"][lead], table.to(DEV), len(rows) // K, K, S, yuv420=layout != "rgb")
        torch.cuda.synchronize()
        _check(got, aug.aug_select_np(src["host"], table.numpy(), len(rows) // K, K, S, layout))


def test_two_calls_give_identical_bytes_and_stats(rgb):
    aug, ops = _aug(), amd("ops")
    S, K = 16, 4
    samples = _samples(RGB_SHAPES, S, K, 7)
    n = len(samples)
    table = aug.make_table([(rgb["offs"][k],) + RGB_SHAPES[k] + (p,) for k, ps in samples for p in ps], S).to(DEV)
    stats = torch.full((3,), 7, dtype=torch.int64, device=DEV)
    a = ops.aug_select(rgb["dev"][0], table, n, K, S, stats=stats)
    b = ops.aug_select(rgb["dev"][0], table, n, K, S, stats=stats)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    _, act = aug.select_candidates_np([rgb["imgs"][k] for k, _ in samples], [ps for _, ps in samples], S)
    assert stats.tolist() == [7 + 2 * int(act.max(axis=1).sum()), 7 + 2 * int(act[:, 0].sum()), 7 + 2 * n]
    c = ops.aug_select(rgb["dev"][0], table, n, K, S)                      # stats NULL: nothing is added anywhere
    assert stats.tolist() == [7 + 2 * int(act.max(axis=1).sum()), 7 + 2 * int(act[:, 0].sum()), 7 + 2 * n]
    assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])


def test_refusals_at_the_c_boundary(rgb):
    C = amd("_C")
    L = C.lib()
    pool = rgb["dev"][0]
    K, n, S = 4, 2, 16
    cand = torch.zeros((1, n * 16, 12), dtype=torch.int64, device=DEV)
    out = torch.zeros((1, n, 12), dtype=torch.int64, device=DEV)
    choice = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    act = torch.full((n * 16,), -9, dtype=torch.int64, device=DEV)
    ws = torch.zeros(n * 17 * 64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(K=K, S=S, n=n, pool_p=p(pool), layout=C.AUG_RGB_HWC, blocks=1, ws_bytes=ws.numel() * 8):
        return L.ofasr_aug_select(pool_p, pool.numel(), p(cand), blocks, n, K, S, layout, p(out), p(choice), p(act), None,
                                  p(ws), ws_bytes, None)

    assert call(K=0) == -2 and b"candidates" in L.ofasr_last_error_string()
    assert call(K=17) == -2
    assert call(S=4097) == -2
    assert call(n=65535 // K + 1) == -2
    assert call(pool_p=None) == -1 and call(n=0) == -1 and call(S=0) == -1 and call(blocks=3) == -1 and call(layout=2) == -1
    assert call(ws_bytes=n * K * 8 - 1) == -3
    torch.cuda.synchronize()
    assert choice.tolist() == [-9] * n and set(act.tolist()) == {-9}       # nothing was launched
    with pytest.raises(C.OfasrError):
        amd("ops").aug_select(pool.cpu(), cand.cpu(), n, K, S)


# ------------------------------------------------------------------------------------------- the loader
def _half_flat(h, w, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    a[:, :w // 2] = 97
    return a


@pytest.mark.parametrize("K", [2, 4, 8])
def test_hand_placed_candidates_through_the_loader(K):
    """the image is half one grey and half noise: the one candidate in the noise wins wherever it stands, 0 .. K - 1;
    of two identical candidates the lower index wins"""
    aug = _aug()
    S = 16
    img = _half_flat(32, 64, 3)
    rs = aug.ResidentArraySet([img, img], DEV)
    loader = aug.ResidentTrainLoader(rs, K + 1, [0] * (K + 1), S, candidates=K, want_f32=True)
    plain = aug.ResidentTrainLoader(rs, K + 1, [0] * (K + 1), S, want_f32=True)
    flat = [(c % 17, (3 * c) % 17, bool(c & 1), 10.0 * c) for c in range(K)]          # all inside the grey half
    detailed = (9, 41, True, -33.3)
    params = [[detailed if c == w else flat[c] for c in range(K)] for w in range(K)]
    params.append([detailed if c in (K // 2, K - 1) else flat[c] for c in range(K)])   # twice the same: the lower index
    idx = [0, 1] * K
    idx = idx[:K + 1]
    batch = loader.batch(idx, params=params)
    assert loader.last_choice.tolist() == list(range(K)) + [K // 2]
    assert loader.last_params == params and loader.last_indices == idx
    act = loader.last_activity.cpu().numpy()
    assert act.shape == (K + 1, K) and act.dtype == np.int64
    want = aug.crop_activity_np(img, detailed, S)
    for w in range(K):
        assert act[w].tolist() == [want if c == w else 0 for c in range(K)]
    ref = plain.batch(idx, params=[detailed] * (K + 1))
    assert set(batch) == set(ref) == {"image_u8", "image"}
    assert torch.equal(batch["image_u8"], ref["image_u8"]) and torch.equal(batch["image"], ref["image"])
    assert np.array_equal(batch["image_u8"][0].cpu().numpy(), aug.apply_params_np(img, S, detailed).transpose(2, 0, 1))
    with pytest.raises(ValueError, match="parameter sets per sample"):
        loader.batch(idx, params=[detailed] * (K + 1))
    with pytest.raises(ValueError):
        aug.ResidentTrainLoader(rs, 2, [0, 1], S, candidates=17)


def test_selection_stats_after_three_batches():
    aug = _aug()
    S, K = 16, 4
    imgs = [_half_flat(40, 56, 1), _half_flat(33, 47, 2), _half_flat(16, 16, 3), _half_flat(24, 64, 4)]
    rs = aug.ResidentArraySet(imgs, DEV)
    loader = aug.ResidentTrainLoader(rs, 2, [0, 1, 2, 3, 1, 0], S, candidates=K)
    assert loader.selection_stats() == (0, 0, 0)
    torch.manual_seed(4)
    chosen = first = count = 0
    for batch in loader:
        choice, act = aug.select_candidates_np([imgs[k] for k in loader.last_indices], loader.last_params, S)
        assert np.array_equal(loader.last_choice.cpu().numpy(), choice)
        assert np.array_equal(loader.last_activity.cpu().numpy(), act)
        chosen, first, count = chosen + int(act.max(axis=1).sum()), first + int(act[:, 0].sum()), count + len(choice)
    assert count == 6 and chosen > first
    assert loader.selection_stats() == (chosen, first, count)
    assert loader.selection_stats() == (0, 0, 0)                           # read and reset
    # the draws: the next K * n of the plain draw, sample-major
    torch.manual_seed(4)
    want = [[aug.draw_train_params(imgs[k].shape[0], imgs[k].shape[1], S) for _ in range(K)] for k in (0, 1)]
    state = torch.get_rng_state()
    torch.manual_seed(4)
    loader.batch([0, 1])
    assert loader.last_params == want and torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------------------------------- the providers
def _epoch(loader):
    """[(indices, params, {key: tensor})] of one pass"""
    return [(loader.last_indices, loader.last_params, b) for b in loader]


def _same_batches(a, b):
    assert len(a) == len(b) > 0
    for (ia, pa, ba), (ib, pb, bb) in zip(a, b):
        assert ia == ib and pa == pb and set(ba) == set(bb)
        for k in ba:
            assert torch.equal(ba[k], bb[k]) if torch.is_tensor(ba[k]) else ba[k] == bb[k], k


def _provider_case(make, srcs_of, hr_params, seed):
    """crop_candidates=4: every batch is the existing gather's for the winners the host statement names;
    crop_candidates=1: the batches of a provider made without the argument, byte for byte, under the same seed"""
    aug = _aug()
    prov = make(crop_candidates=4)
    loader = prov.train
    assert loader.candidates == 4
    S = loader.size
    plain = aug.ResidentTrainLoader(prov.resident_set, loader.batch_size, loader.sampler, S, want_f32=True)
    torch.manual_seed(seed)
    seen = 0
    for batch in loader:
        idx, cands = loader.last_indices, loader.last_params
        assert all(len(c) == 4 for c in cands)
        choice, act = aug.select_candidates_np(srcs_of(prov.resident_set, idx), [[hr_params(p) for p in c] for c in cands], S)
        assert np.array_equal(loader.last_choice.cpu().numpy(), choice)
        assert np.array_equal(loader.last_activity.cpu().numpy(), act)
        ref = plain.batch(idx, params=[c[w] for c, w in zip(cands, choice)])
        assert set(ref) == set(batch)
        for k in ref:
            assert torch.equal(batch[k], ref[k]) if torch.is_tensor(ref[k]) else batch[k] == ref[k], k
        seen += len(idx)
    assert seen == len(loader) * loader.batch_size > 0
    assert loader.selection_stats()[2] == seen
    one, none = make(crop_candidates=1), make()
    assert one.train.candidates == none.train.candidates == 1
    torch.manual_seed(seed + 1)
    a = _epoch(one.train)
    torch.manual_seed(seed + 1)
    b = _epoch(none.train)
    _same_batches(a, b)
    assert one.train.last_choice is None and one.train.selection_stats() == (0, 0, 0)
    # the sub-train loader is the plain one
    sub = prov.build_sub_train_loader(3, 2)
    assert [b["image_u8"].shape[0] for b in sub] == [2, 1]


def test_div2k_provider_end_to_end(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    (tmp_path / "train").mkdir()
    (tmp_path / "val").mkdir()
    for k, (h, w) in enumerate([(16, 16), (23, 31), (40, 17), (33, 48), (19, 64)]):
        Image.fromarray(_half_flat(h, w, 50 + k)).save(str(tmp_path / "train" / ("t%d.png" % k)))
    for k, (h, w) in enumerate([(21, 18), (16, 30)]):
        Image.fromarray(_half_flat(h, w, 60 + k)).save(str(tmp_path / "val" / ("v%d.png" % k)))
    torch.cuda.set_device(0)
    kw = dict(save_path=str(tmp_path), train_batch_size=2, test_batch_size=1, n_worker=0, image_size=16, resident=True)
    _provider_case(lambda **k: dp.Div2K_SetXXDataProvider(**dict(kw, **k)),
                   lambda rs, idx: [rs.image_np(k) for k in idx], lambda p: p, 31)
    with pytest.raises(ValueError, match="resident pool"):
        dp.Div2K_SetXXDataProvider(**dict(kw, resident=False, crop_candidates=4))


def test_video_provider_end_to_end(tmp_path):
    vf = amd("imagenet_codebase.data_providers.video_frames")
    path = str(tmp_path / "clip.y4m")
    write_video(path, 7, 38, 54, seed=8)
    torch.cuda.set_device(0)
    kw = dict(videos=[path], valid_every=3, test_batch_size=1, image_size=16, train_batch_size=2)
    _provider_case(lambda **k: vf.VideoFramesDataProvider(**dict(kw, **k)),
                   lambda rs, idx: [rs.frame_planes_np(k)[0] for k in idx], lambda p: p, 41)


@pytest.mark.parametrize("f", [2, 4])
def test_pair_provider_end_to_end(tmp_path, f):
    aug = _aug()
    vf = amd("imagenet_codebase.data_providers.video_frames")
    (H, W), (h, w) = {4: ((64, 64), (16, 16)), 2: ((64, 96), (32, 48))}[f]
    hr, lr = str(tmp_path / "hr.y4m"), str(tmp_path / "lr.y4m")
    write_video(hr, 6, H, W, seed=20 + f)
    write_video(lr, 6, h, w, seed=30 + f)
    torch.cuda.set_device(0)
    kw = dict(videos=[hr], videos_lr=[lr], valid_every=3, test_batch_size=1, image_size=32, train_batch_size=2)
    _provider_case(lambda **k: vf.VideoFramesDataProvider(**dict(kw, **k)),
                   lambda rs, idx: [rs.frame_planes_np(k)[0] for k in idx], lambda p: aug.pair_hr_params(p, f), 51)
