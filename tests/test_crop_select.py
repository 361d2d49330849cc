"""Best of K candidate training crops, the host side (data_providers/augment.py): the measure is routing.py's, the draws
are the existing draws K times per sample, ties keep the lowest index, and aug_select_np -- the kernel restated on the
pool's bytes -- equals the plain statement inside the contract and obeys the stated clamps outside it.  No GPU."""
import numpy as np
import pytest
import torch

from conftest import amd


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _half_flat(h, w, seed, rgb=True):
    """left half one grey, right half noise"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (h, w, 3) if rgb else (h, w)).astype(np.uint8)
    a[:, :w // 2] = 97
    return a


def test_activity_is_routings_window_activity():
    aug, routing = _aug(), amd("routing")
    rng = np.random.RandomState(1)
    for shape in [(40, 56, 3), (33, 47, 3), (38, 54), (64, 48)]:
        src = rng.randint(0, 256, shape).astype(np.uint8)
        for S in (1, 2, 15, 16, min(shape[:2])):
            for _ in range(6):
                i, j = rng.randint(0, shape[0] - S + 1), rng.randint(0, shape[1] - S + 1)
                a = aug.crop_activity_np(src, (i, j, False, 0.0), S)
                assert a == int(routing.window_activity_host(src, [(i, j)], S, S)[0])
                assert 0 <= a <= 510 * S * S
    with pytest.raises(ValueError):
        aug.crop_activity_np(np.zeros((8, 8), np.uint8), (1, 0, False, 0.0), 8)


def test_one_candidate_consumes_the_rng_as_the_plain_draws():
    aug = _aug()
    shapes = [(40, 56), (33, 47), (16, 16), (40, 56)]
    torch.manual_seed(11)
    plain = [aug.draw_train_params(h, w, 16) for (h, w) in shapes]
    after = torch.rand(1).item()
    torch.manual_seed(11)
    cands = [aug.draw_candidates(lambda: aug.draw_train_params(h, w, 16), 1) for (h, w) in shapes]
    assert [c[0] for c in cands] == plain and all(len(c) == 1 for c in cands)
    assert torch.rand(1).item() == after
    # the paired draw, on its LR grid
    torch.manual_seed(12)
    plain = [aug.draw_pair_params(20, 28, 16, 2, rotate=False) for _ in range(3)]
    after = torch.rand(1).item()
    torch.manual_seed(12)
    cands = [aug.draw_candidates(lambda: aug.draw_pair_params(20, 28, 16, 2, rotate=False), 1) for _ in range(3)]
    assert [c[0] for c in cands] == plain
    assert torch.rand(1).item() == after


def test_three_candidates_are_the_next_draws_sample_major():
    aug = _aug()
    shapes = [(40, 56), (33, 47), (16, 16)]
    torch.manual_seed(5)
    flat = [aug.draw_train_params(h, w, 16) for (h, w) in shapes for _ in range(3)]
    torch.manual_seed(5)
    cands = [aug.draw_candidates(lambda: aug.draw_train_params(h, w, 16), 3) for (h, w) in shapes]
    assert [p for c in cands for p in c] == flat
    for K in (0, 17):
        with pytest.raises(ValueError):
            aug.draw_candidates(lambda: None, K)


def test_ties_go_to_the_lowest_index_and_flat_images_keep_the_first_draw():
    aug = _aug()
    flat = np.full((32, 32, 3), 200, np.uint8)
    cands = [[(0, 0, False, 0.0), (5, 7, True, 30.0), (16, 16, False, -45.0)]]
    choice, act = aug.select_candidates_np([flat], cands, 16)
    assert choice.dtype == np.int32 and act.dtype == np.int64
    assert choice.tolist() == [0] and act.tolist() == [[0, 0, 0]]
    img = _half_flat(32, 64, 2)
    # candidates 1 and 2 are the same rectangle (different flip / angle: the measure is taken before both)
    cands = [[(0, 0, False, 0.0), (8, 40, False, 0.0), (8, 40, True, 77.0), (0, 1, False, 0.0)]]
    choice, act = aug.select_candidates_np([img], cands, 16)
    assert act[0, 1] == act[0, 2] > 0 and act[0, 0] == 0 == act[0, 3]
    assert choice.tolist() == [1]


def test_strip_function():
    aug = _aug()
    assert [aug.aug_select_strips(S) for S in (1, 16, 128, 129, 256, 1024, 4096)] == [1, 1, 1, 2, 4, 64, 64]


def _pool(images):
    offs = np.cumsum([0] + [a.size for a in images])
    return np.concatenate([a.reshape(-1) for a in images]), [int(o) for o in offs[:-1]]


@pytest.mark.parametrize("S,K", [(16, 1), (15, 3), (16, 4)])
def test_pool_statement_equals_the_plain_statement_rgb(S, K):
    aug = _aug()
    imgs = [_half_flat(40, 56, 3), _half_flat(33, 47, 4), _half_flat(16, 16, 5)]
    if S != 16:
        imgs = imgs[:2]
    pool, offs = _pool(imgs)
    torch.manual_seed(S * 100 + K)
    idx = [0, 1, len(imgs) - 1, 0, 1]
    cands = [aug.draw_candidates(lambda: aug.draw_train_params(imgs[k].shape[0], imgs[k].shape[1], S), K) for k in idx]
    table = aug.make_table([(offs[k],) + imgs[k].shape[:2] + (p,) for k, c in zip(idx, cands) for p in c], S).numpy()
    choice, act, out = aug.aug_select_np(pool, table, len(idx), K, S, aug.LAYOUT_RGB)
    ref_choice, ref_act = aug.select_candidates_np([imgs[k] for k in idx], cands, S)
    assert np.array_equal(choice, ref_choice) and np.array_equal(act, ref_act)
    assert choice.dtype == np.int32 and act.dtype == np.int64 and out.shape == (1, len(idx), 12)
    want = aug.make_table([(offs[k],) + imgs[k].shape[:2] + (c[w],) for k, c, w in zip(idx, cands, choice)], S).numpy()
    assert np.array_equal(out[0], want)


@pytest.mark.parametrize("f", [2, 4])
def test_pool_statement_equals_the_plain_statement_yuv_and_pair(f):
    aug = _aug()
    S, K = 16, 3
    H, W = 48, 64
    rng = np.random.RandomState(f)
    frames = []
    for s in range(2):
        y = _half_flat(H, W, 20 + s, rgb=False)
        frames.append((y, rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8),
                       rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8)))
    fb = H * W * 3 // 2
    pool = np.concatenate([np.concatenate([p.reshape(-1) for p in fr]) for fr in frames])
    lr_fb = (H // f) * (W // f) * 3 // 2
    torch.manual_seed(40 + f)
    idx = [1, 0, 1]
    cands = [aug.draw_candidates(lambda: aug.draw_pair_params(H // f, W // f, S, f), K) for _ in idx]
    rows = [(k * fb, H, W, k * lr_fb, H // f, W // f, p) for k, c in zip(idx, cands) for p in c]
    table = aug.make_pair_table(rows, S, f).numpy()
    assert table.shape == (2, len(idx) * K, 12)
    choice, act, out = aug.aug_select_np(pool, table, len(idx), K, S, aug.LAYOUT_YUV420)
    hr = [[aug.pair_hr_params(p, f) for p in c] for c in cands]
    ref_choice, ref_act = aug.select_candidates_np([frames[k][0] for k in idx], hr, S)
    assert np.array_equal(choice, ref_choice) and np.array_equal(act, ref_act)
    want = aug.make_pair_table([(k * fb, H, W, k * lr_fb, H // f, W // f, c[w]) for k, c, w in zip(idx, cands, choice)],
                               S, f).numpy()
    assert out.shape == (2, len(idx), 12) and np.array_equal(out, want)     # both blocks of the winner
    # an unpaired 4:2:0 table is block 0 alone
    c1, a1, o1 = aug.aug_select_np(pool, table[0], len(idx), K, S, aug.LAYOUT_YUV420)
    assert np.array_equal(c1, choice) and np.array_equal(a1, act) and np.array_equal(o1[0], out[0])


@pytest.mark.parametrize("layout", ["rgb", "yuv420"])
def test_pool_statement_obeys_the_clamps(layout):
    """out-of-contract rows: the activities are those of the stated clamps, restated here byte address by byte address
    with every address asserted inside the pool (the pool is noise, so equal sums mean equal reads)"""
    aug = _aug()
    S, K = 16, 4
    rng = np.random.RandomState(9)
    pool = rng.randint(0, 256, 40 * 56 * 3).astype(np.uint8)
    nb, bps, yuv = pool.size, (3 if layout == "rgb" else 1), layout == "yuv420"
    ident = (65536, 0, 32768, 0, 65536, 32768)
    rows = [(-5, 40, 56, 3, 4, 0) + ident,                 # a negative offset -> 0
            (0, 40, 56, 40, 56, 1) + ident,                # i > H - S, j > W - S -> the last corner
            (0, 1 << 40, 1 << 40, 7, 9, 0) + ident,        # a huge H, W -> 2^24: addresses far outside, clamped per byte
            (nb + 100, 5, 5, -3, -3, 0) + ident]           # offset -> pool bytes, H, W -> S, i, j -> 0
    table = np.array(rows, dtype=np.int64).reshape(1, K, 12)
    choice, act, out = aug.aug_select_np(pool, table, 1, K, S, layout)
    r, c = np.mgrid[0:S, 0:S].astype(np.int64)
    Se = (S + 1) & ~1 if yuv else S
    for q, row in enumerate(rows):
        off, H, W, i, j = row[:5]
        H, W = min(max(H, Se), 1 << 24), min(max(W, Se), 1 << 24)
        if yuv:
            H, W = H & ~1, W & ~1
        i, j = min(max(i, 0), H - S), min(max(j, 0), W - S)
        off = min(max(off, 0), nb)
        assert 0 <= i <= H - S and 0 <= j <= W - S and 0 <= off <= nb
        raw = off + ((i + r) * W + j + c) * bps
        a, a1, a2 = (np.minimum(raw + b, nb - 1) for b in range(3))
        assert raw.min() >= 0 and max(a.max(), a1.max(), a2.max()) <= nb - 1
        p64 = pool.astype(np.int64)
        L = p64[a] if yuv else (77 * p64[a] + 150 * p64[a1] + 29 * p64[a2] + 128) >> 8
        want = int(np.abs(np.diff(L, axis=1)).sum()) + int(np.abs(np.diff(L, axis=0)).sum())
        assert act[0, q] == want
    assert act[0, 3] == 0                                  # every byte of the row at the pool's end is the last byte
    assert choice[0] == int(np.argmax(act[0])) and np.array_equal(out[0, 0], table[0, choice[0]])   # the row, unclamped
    # row 1 is the in-contract row at the last corner
    img = pool.reshape(40, 56, 3) if not yuv else pool[:40 * 56].reshape(40, 56)
    assert act[0, 1] == aug.crop_activity_np(img, (40 - S, 56 - S, False, 0.0), S)
    with pytest.raises(ValueError):
        aug.aug_select_np(pool, table, 1, K, S, "nv12")


def test_loader_and_provider_refusals_without_a_gpu():
    aug = _aug()
    rm = amd("imagenet_codebase.run_manager")
    with pytest.raises(ValueError):
        aug.check_candidates(0)
    with pytest.raises(ValueError):
        aug.check_candidates(17)
    with pytest.raises(ValueError, match="resident"):
        rm.Div2K_SetXXRunConfig(crop_candidates=4)
    cfg = rm.Div2K_SetXXRunConfig(crop_candidates=4, resident=True)
    assert cfg.config["crop_candidates"] == 4
    assert "crop_candidates" not in rm.Div2K_SetXXRunConfig(resident=True).config     # K = 1: the config is what it was
    assert "crop_candidates" not in rm.VideoFramesRunConfig(videos=["a.y4m"]).config
    assert rm.VideoFramesRunConfig(videos=["a.y4m"], crop_candidates=2).config["crop_candidates"] == 2
