"""-m gpu: the one-pass recipe -- a colour stage on source pixels (HED or HSB), a view of any kind and the post stage on written pixels in
ONE launch: sl_normalize_stages_view / _view_affine / _view_elastic, engine.normalize_stages_view*, stainlib_amd.Recipe and recipe= on the
batch methods.

The definition is a composition of definitions that exist (include/stainlib_hip.h):  out = convert(post(view(colour(full)))).  The
oracle is built from them and from nothing new: `full` is what engine.normalize_view writes through the identity window; colour is
augmentation.hsb.hsb_reference, or -- HED's arithmetic is binary32 on the device -- the existing engine.normalize_hed_view without a view;
the view is tile_view.view_planes_reference (window, box shrink, area resample, flip and turn), affine_resample or elastic_resample; post is
augmentation.noise.post_reference with p counted in the view's output.  Every comparison is exact.

Shapes: N = 4 tiles of 149 x 171 (P % 4 != 0, tile bases unaligned), output 67 x 81: two patches a side at the identity (63 + 4 rows,
63 + 18 columns with a ragged last lane), more under a rotation and under max_d = 4 with cell = 16.  Tile 0: the identity row and a zero
field, the identity table and sigma 64; tile 1: 45 degrees, zoomed out 1.3 times, centred near a corner -- taps straddle the tile's edge
and whole patches miss it --, zero HSB codes, hed_applied = 0; tile 2: all white, its fit fails (the recipe on its own bytes), a
permutation table; tile 3: a drawn row with a drawn field at the bound.  Outputs go into guarded buffers whose sentinels are checked."""
import numpy as np
import pytest
import torch

import stainlib_amd
from oracle import stain_oracle as so
from stainlib_amd import engine
from stainlib_amd.augmentation.hsb import hsb_codes, hsb_reference
from stainlib_amd.augmentation.noise import noise_codes, post_reference
from stainlib_amd.tile_view import (AFFINE_Q as Q, ElasticWindows, affine_resample, affine_row_sums, elastic_grid_shape, elastic_nearest,
                                    elastic_resample, view_planes_reference)
from tests.big_batch import guarded
from tests.test_gpu_hsb import FORMATS
from tests.test_gpu_jitter import MEAN, STD, _same_bits
from tests.test_gpu_post import _chain, _stage
from tests.test_gpu_view_affine import _dihedral_row, _rot, _row

pytestmark = pytest.mark.gpu

N, H, W = 4, 149, 171
SIZE = (67, 81)
FILL = (10, 30, 200)
CELL, MAX_D = 16, 4
ROUTES = ["raw", "apply", "jitter_tissue", "jitter_all"]
KINDS = ["affine", "elastic", "fixed", "shrink2", "scale"]
COLOURS = ["hed", "hsb", "none"]
POSTS = ["tone", "noise", "both", "mono"]                     # (_stage of tests/test_gpu_post.py: tile 0 identity / sigma 64, tile 2 a permutation)
# every dtype in both layouts: with the uint8 image the seven output forms a kernel family is instantiated for (FORMATS is four of them)
ALL_FORMATS = tuple(stainlib_amd.TensorFormat(dtype=dt, channels_last=cl, mean=MEAN, std=STD)
                    for dt in (torch.float16, torch.bfloat16, torch.float32) for cl in (False, True))
_CACHE = {}


def _fmt_id(f):
    return "u8" if f is None else str(f.dtype).split(".")[1] + ("_nhwc" if f.channels_last else "")


def _setup():
    """the tiles, their fit, the four routes and `full` of each route (the identity window through the EXISTING view pass)"""
    if "setup" not in _CACHE:
        t = np.stack([so.synth_tile(H, W, 40 + 7 * i) for i in range(N)])
        t[2] = 255
        t[2, 10:20, 10:30] = (250, 240, 245)
        dev = torch.from_numpy(t).cuda()
        M, maxC, status = engine.macenko_fit(dev)
        assert int(status[2]) != 0 and status[[0, 1, 3]].cpu().tolist() == [0, 0, 0]
        nz = stainlib_amd.MacenkoNormalizer()
        nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
        Mt, ct = nz._target_on(dev.device)
        np.random.seed(9)
        ab = stainlib_amd.StainJitter().draw(N)
        fit = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct)
        routes = {"raw": {}, "apply": fit, "jitter_tissue": dict(alpha_beta=ab, **fit),
                  "jitter_all": dict(alpha_beta=ab, augment_background=True, **fit)}
        ident = np.zeros((N, 3), dtype=np.int32)
        full = {r: engine.normalize_view(dev, ident, None, 0, **routes[r]) for r in ROUTES}
        assert torch.equal(full["raw"], dev) and torch.equal(full["apply"][2], dev[2]) and not torch.equal(full["apply"][0], dev[0])
        _CACHE["setup"] = (dev, routes, full)
    return _CACHE["setup"]


def _colour_args(colour):
    """the stage keywords of a colour stage: hed_applied[1] = 0; the HSB codes of tile 1 are zero"""
    if colour == "none":
        return {}
    rng = np.random.RandomState(21)
    if colour == "hed":
        return dict(hed_sigma=rng.uniform(-0.2, 0.2, (N, 3)), hed_bias=rng.uniform(-0.05, 0.05, (N, 3)),
                    hed_applied=np.array([1, 0, 1, 1], dtype=np.int32))
    sg = np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(-0.3, 0.3, N), rng.uniform(-0.3, 0.3, N)], axis=1)
    sg[1] = 0.0
    codes = hsb_codes(sg)
    assert not codes[1].any() and codes[0].any()
    return dict(hsb_codes=codes)


def _post_args(post):
    if post == "none":
        return {}
    tables, codes = _stage(N, post)
    return {k: v for k, v in (("tables", tables), ("codes", codes)) if v is not None}


def _coloured(route, colour):
    """colour(full) of a route, (N, H, W, 3) uint8 numpy: hsb_reference, or the existing HED call without a view"""
    key = ("colour", route, colour)
    if key not in _CACHE:
        dev, routes, full = _setup()
        if colour == "none":
            img = full[route].cpu().numpy()
        elif colour == "hsb":
            img = hsb_reference(full[route].cpu().numpy(), _colour_args("hsb")["hsb_codes"])
        else:
            a = _colour_args("hed")
            img = engine.normalize_hed_view(dev, np.zeros((N, 3), dtype=np.int32), None, 0, a["hed_sigma"], a["hed_bias"], a["hed_applied"],
                                            **routes[route]).cpu().numpy()
            assert np.array_equal(img[1], full[route][1].cpu().numpy()) and not np.array_equal(img[0], full[route][0].cpu().numpy())
        _CACHE[key] = img
    return _CACHE[key]


def _affine_rows():
    if "rows" not in _CACHE:
        np.random.seed(31)
        drawn = stainlib_amd.TileAffine(SIZE, zoom=(0.8, 1.3), shear=(-8, 8), translate=(0.3, 0.3), fill=FILL).draw(N, H, W)
        rows = np.array([_row(H / 2, W / 2, 1, 0, 0, 1), _row(12.3, W - 9.6, *_rot(45, 1 / 1.3)), _row(H / 2 + 0.5, W / 2 + 0.25, *_rot(30)),
                         drawn[3].tolist()], dtype=np.int64)
        assert int(affine_row_sums(rows).max()) <= 2 * Q
        _CACHE["rows"] = rows.astype(np.int32)
    return _CACHE["rows"]


def _field():
    """tile 0 zero, tile 3 every control value at the bound +-256 max_d, the others drawn"""
    if "field" not in _CACHE:
        gh, gw = elastic_grid_shape(SIZE, CELL)
        rng = np.random.RandomState(33)
        f = rng.randint(-256 * MAX_D, 256 * MAX_D + 1, (N, gh, gw, 2)).astype(np.int32)
        f[0] = 0
        f[3] = 256 * MAX_D * rng.choice([-1, 1], (gh, gw, 2))
        _CACHE["field"] = f
    return _CACHE["field"]


def _tile_view(kind):
    if kind == "fixed":
        return stainlib_amd.TileView(SIZE), np.array([(0, 0, 0), (H - 81, W - 67, 5), (41, 45, 6), (3, 2, 3)], dtype=np.int32)
    if kind == "shrink2":                                        # a 134 x 162 window does not fit turned: no quarter turns
        return stainlib_amd.TileView(SIZE, shrink=2, rot90=False), np.array([(0, 0, 0), (15, 9, 4), (7, 3, 2), (15, 0, 6)], dtype=np.int32)
    if "scale" not in _CACHE:
        view = stainlib_amd.TileView(SIZE, scale=(0.3, 1))
        np.random.seed(5)
        _CACHE["scale"] = (view, view.draw(N, H, W))
        assert _CACHE["scale"][1].shape == (N, 5)
    return _CACHE["scale"]


def _viewed(kind, route, colour):
    """view(colour(full)), (N, 67, 81, 3) uint8 numpy, by the numpy definition of the view's type"""
    key = ("view", kind, route, colour)
    if key not in _CACHE:
        img = _coloured(route, colour)
        if kind == "affine":
            out = np.stack([affine_resample(img[t], _affine_rows()[t], SIZE, FILL) for t in range(N)])
        elif kind == "elastic":
            out = np.stack([elastic_resample(img[t], _affine_rows()[t], _field()[t], SIZE, CELL, FILL) for t in range(N)])
        else:
            view, win = _tile_view(kind)
            out = view_planes_reference(img.transpose(0, 3, 1, 2), win, SIZE, shrink=view.shrink, mode="area").transpose(0, 2, 3, 1)
        _CACHE[key] = np.ascontiguousarray(out)
    return _CACHE[key]


def _call(kind, dev, fmt, out, route, stages, windows=None, field=None, max_r=None):
    """the engine call of a view kind (host windows unless given)"""
    if kind in ("affine", "elastic"):
        win = _affine_rows() if windows is None else windows
        max_r = int(affine_row_sums(_affine_rows()).max()) if max_r is None else max_r
        if kind == "affine":
            return engine.normalize_stages_view_affine(dev, win, SIZE, max_r, FILL, fmt=fmt, out=out, **route, **stages)
        return engine.normalize_stages_view_elastic(dev, win, _field() if field is None else field, SIZE, CELL, max_r, MAX_D, FILL, fmt=fmt,
                                                    out=out, **route, **stages)
    view, win = _tile_view(kind)
    win = win if windows is None else windows
    return engine.normalize_stages_view(dev, win, SIZE, view.d_mask, fmt=fmt, out=out, shrink=view.shrink,
                                        resize=engine._view_resize(view, win, dev), **route, **stages)


def _guarded_call(kind, dev, fmt, route, stages, **kw):
    g = guarded(N * SIZE[0] * SIZE[1] * 3, fmt.dtype if fmt is not None else torch.uint8)
    out = g.image(N, SIZE[0], SIZE[1], fmt)
    res = _call(kind, dev, fmt, out, route, stages, **kw)
    g.check(f"{kind} {_fmt_id(fmt)}")
    assert res.data_ptr() == out.data_ptr()
    return res.cpu()


# ---- 1. the three engine calls against the composed oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("kind", KINDS)
def test_engine_calls_are_the_composition_bit_for_bit(kind, colour):
    """every post variant on the four routes as uint8 and in every format of FORMATS on one route; beyond that every (route, output form)
    pair once per kernel family -- with the post stage and, for a colour stage, without it -- so that each of a family's 28 instantiations
    is launched"""
    dev, routes, _ = _setup()
    posts = POSTS + (["none"] if colour != "none" else [])
    launched = {True: set(), False: set()}
    for vi, post in enumerate(posts):
        stages = dict(**_colour_args(colour), **_post_args(post))
        for ri, rname in enumerate(ROUTES):
            u8 = _viewed(kind, rname, colour)
            want8 = torch.from_numpy(post_reference(u8, tables=stages.get("tables"), codes=stages.get("codes")) if post != "none" else u8)
            if post != "none" and rname == "raw":
                assert not torch.equal(want8, torch.from_numpy(u8))
            fmts = [None] + [f for f in FORMATS[1:] if ri == vi % 4]
            fmts += [f for fi, f in enumerate(ALL_FORMATS) if post == "none" or (fi + ri) % len(POSTS) == vi]
            for fmt in fmts:
                got = _guarded_call(kind, dev, fmt, routes[rname], stages)
                launched[post != "none"].add((rname, _fmt_id(fmt)))
                if fmt is None:
                    assert got.dtype == torch.uint8 and torch.equal(got, want8), (kind, colour, post, rname)
                else:
                    assert tuple(got.shape) == (N, 3) + SIZE and _same_bits(got, fmt.convert(want8.cuda()).cpu()), (kind, colour, post, rname, fmt)
    for with_post in ((True, False) if colour != "none" else (True,)):
        assert len(launched[with_post]) == 28, (with_post, sorted(launched[with_post]))
    if kind in ("affine", "elastic"):                             # the oracle has fill pixels, and a tile's own bytes where its fit failed
        u8 = _viewed(kind, "apply", colour)
        assert (u8[1] == np.array(FILL, dtype=np.uint8)).all(axis=-1).mean() > 0.3 and not (u8[0] == np.array(FILL, dtype=np.uint8)).all(axis=-1).any()
        assert np.array_equal(_viewed(kind, "apply", "none")[2], _viewed(kind, "raw", "none")[2])


@pytest.mark.parametrize("kind", ["affine", "elastic"])
def test_device_windows_beyond_max_r_are_all_fill_then_post(kind):
    """device windows are taken as they are: a tile whose row sums pass the call's max_r is written as fill -- which does not take the colour
    stage and does take the post stage; the other tiles are unchanged"""
    dev, routes, _ = _setup()
    rows = _affine_rows()
    sums = affine_row_sums(rows)
    big = int(np.argmax(sums))
    max_r = int(np.sort(sums)[-2])                               # the second largest: tile `big` alone is beyond it
    assert sums[big] > max_r and (np.delete(sums, big) <= max_r).all()
    stages = dict(**_colour_args("hsb"), **_post_args("both"))
    for rname in ("raw", "jitter_tissue"):
        u8 = _viewed(kind, rname, "hsb").copy()
        u8[big] = np.array(FILL, dtype=np.uint8)
        want = torch.from_numpy(post_reference(u8, tables=stages["tables"], codes=stages["codes"]))
        for fmt in (None, FORMATS[1]):
            got = _guarded_call(kind, dev, fmt, routes[rname], stages, windows=torch.from_numpy(rows).cuda(),
                                field=torch.from_numpy(_field()).cuda(), max_r=max_r)
            assert _same_bits(got, want if fmt is None else fmt.convert(want.cuda()).cpu()), (kind, rname, fmt)
    assert not (want[big] == torch.tensor(FILL, dtype=torch.uint8)).all()                       # (the post stage moved the fill)


# ---- 2. the affine recipe on signed permutations is the TileView recipe; the elastic one on a zero field is the affine one -------------------
def test_dihedral_rows_are_the_tile_view_recipe_and_a_zero_field_is_the_affine_recipe():
    dev, routes, _ = _setup()
    idx = torch.tensor([0, 1, 2, 3, 3, 2, 1, 0], device="cuda")
    dev8 = dev[idx].contiguous()
    r = routes["jitter_tissue"]
    route8 = dict(M_src=r["M_src"][idx].contiguous(), maxC_src=r["maxC_src"][idx].contiguous(), M_tgt=r["M_tgt"], maxC_tgt=r["maxC_tgt"],
                  alpha_beta=np.asarray(r["alpha_beta"])[idx.cpu().numpy()])
    tables, codes = _stage(8, "both")
    hc = np.tile(_colour_args("hsb")["hsb_codes"], (2, 1))
    stages = dict(hsb_codes=hc, tables=tables, codes=codes)
    win3 = np.array([(5 + d, 3 + d, d) for d in range(8)], dtype=np.int32)
    win6 = np.array([_dihedral_row(5 + d, 3 + d, d, SIZE) for d in range(8)], dtype=np.int32)
    for route in ({}, route8):
        for fmt in (None, FORMATS[2]):
            want = engine.normalize_stages_view(dev8, win3, SIZE, 7, fmt=fmt, **route, **stages).cpu()
            got = engine.normalize_stages_view_affine(dev8, win6, SIZE, Q, FILL, fmt=fmt, **route, **stages).cpu()
            assert _same_bits(got, want), (bool(route), fmt)         # p counts in the OUTPUT: the noise of a turned tile is not turned
            zero = np.zeros((8,) + elastic_grid_shape(SIZE, CELL) + (2,), dtype=np.int32)
            for max_d in (0, MAX_D):
                gz = engine.normalize_stages_view_elastic(dev8, win6, zero, SIZE, CELL, Q, max_d, FILL, fmt=fmt, **route, **stages).cpu()
                assert _same_bits(gz, want), (bool(route), fmt, max_d)
    # the identity about the centre of the full tile: the stages on the full tile, nothing else
    ident = np.array([_row(H / 2, W / 2, 1, 0, 0, 1)] * N, dtype=np.int32)
    st4 = dict(hsb_codes=hc[:N], tables=tables[:N], codes=codes[:N])
    want = engine.normalize_stages_view(dev, np.zeros((N, 3), dtype=np.int32), None, 0, **routes["apply"], **st4)
    assert torch.equal(engine.normalize_stages_view_affine(dev, ident, None, Q, FILL, **routes["apply"], **st4), want)


# ---- 3. neutral stages are today's calls --------------------------------------------------------------------------------------------------
def test_neutral_stages_are_todays_affine_and_elastic_bits():
    dev, routes, _ = _setup()
    rows, field = _affine_rows(), _field()
    max_r = int(affine_row_sums(rows).max())
    ident = np.tile(np.arange(256, dtype=np.uint8), (N, 1))
    sq0 = noise_codes(np.zeros(N), np.arange(2 * N).reshape(N, 2))
    assert not sq0[:, 0].any() and sq0[:, 1:3].any()
    rng = np.random.RandomState(3)
    neutral = [dict(tables=ident), dict(codes=sq0), dict(tables=ident, codes=sq0), dict(hsb_codes=np.zeros((N, 3), dtype=np.int32)),
               dict(hsb_codes=np.zeros((N, 3), dtype=np.int32), tables=ident, codes=sq0),
               dict(hed_sigma=rng.uniform(-0.2, 0.2, (N, 3)), hed_bias=rng.uniform(-0.05, 0.05, (N, 3)), hed_applied=np.zeros(N, dtype=np.int32)),
               dict(hed_sigma=rng.uniform(-0.2, 0.2, (N, 3)), hed_bias=rng.uniform(-0.05, 0.05, (N, 3)), hed_applied=np.zeros(N, dtype=np.int32),
                    tables=ident)]
    for rname in ROUTES:
        for fmt in (None, FORMATS[1]):
            wa = engine.normalize_view_affine(dev, rows, SIZE, max_r, FILL, fmt=fmt, **routes[rname]).cpu()
            we = engine.normalize_view_elastic(dev, rows, field, SIZE, CELL, max_r, MAX_D, FILL, fmt=fmt, **routes[rname]).cpu()
            assert not _same_bits(wa, we)
            for st in neutral:
                assert _same_bits(engine.normalize_stages_view_affine(dev, rows, SIZE, max_r, FILL, fmt=fmt, **routes[rname], **st).cpu(), wa), (rname, fmt, sorted(st))
                assert _same_bits(engine.normalize_stages_view_elastic(dev, rows, field, SIZE, CELL, max_r, MAX_D, FILL, fmt=fmt, **routes[rname],
                                                                       **st).cpu(), we), (rname, fmt, sorted(st))


# ---- 4. recipe= on the public methods: each against the chain of existing method calls fed the returned draws -------------------------------
def _f16():
    return stainlib_amd.TensorFormat(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD)


def _colour_kw(color, draw):
    """the existing keywords that reproduce a recipe's colour stage from its draw"""
    if color is None:
        return {}
    if isinstance(draw, engine.HedDraw):
        return dict(hed=color, hed_sigmas=draw.sigmas, hed_biases=draw.biases)
    return dict(hsb=color, hsb_sigmas=draw.sigmas)


def _chain_of(full_call, recipe, draw, fmt):
    """colour on the full tile (an existing keyword), the view to uint8 (engine.view_pass), tone and noise behind it (test_gpu_post._chain)"""
    u8 = full_call(**_colour_kw(recipe.color, draw.color))[0]
    assert u8.dtype == torch.uint8
    if recipe.view is not None:
        u8 = engine.view_pass(u8, recipe.view, draw.windows)[0]
    if draw.post is None:
        return u8 if fmt is None else fmt.convert(u8)
    return _chain(u8, draw.post, fmt)


def _to_device(draw):
    """the same draw with every array that may live on the device moved there"""
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None      # noqa: E731
    win = draw.windows
    if isinstance(win, ElasticWindows):
        win = ElasticWindows(dv(win.affine), dv(win.field))
    elif win is not None:
        win = dv(win)
    color = draw.color
    if isinstance(color, engine.HsbDraw):
        color = engine.HsbDraw(color.sigmas, dv(color.codes))
    post = draw.post
    if post is not None:
        post = engine.PostDraw(post.tone_params, dv(post.tone_tables), post.noise_sigmas, dv(post.noise_codes))
    return engine.RecipeDraw(win, color, post)


def _recipes():
    hsb = stainlib_amd.HsbLightColorAugmenter()
    hed = stainlib_amd.HedLightColorAugmenter()
    noise = stainlib_amd.GaussianNoiseAugmenter((1, 12), per_channel=False)
    tone = stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), (0.8, 1.25), (0.7, 1.4))
    el = stainlib_amd.TileElastic(48, rotate=(-180, 180), zoom=(0.8, 1.25), magnitude=(1, 4), cell=16, fill=FILL)
    af = stainlib_amd.TileAffine((40, 33), zoom=(0.8, 1.3), shear=(-8, 8), fill=FILL)
    R = stainlib_amd.Recipe
    return [R(el, hsb, noise, tone), R(af, hed, noise, None), R(el, hed, None, tone), R(af, hsb), R(el, None, noise),
            R(stainlib_amd.TileView(48), hsb, noise, tone), R(stainlib_amd.TileView(24, shrink=2), hed, None, tone),
            R(stainlib_amd.TileView((40, 33), scale=(0.4, 1)), hsb, noise), R(None, hed, noise, tone), R(None, hsb), R(None, None, noise)]


def _class_batch():
    t = np.stack([so.synth_tile(64, 64, 40 + 7 * i) for i in range(5)] + [np.full((64, 64, 3), 255, dtype=np.uint8)])
    t[5, 10:20, 10:20] = (250, 240, 245)
    return torch.from_numpy(t).cuda()


def _check_method(call, full_call, recipe, fmt, base, tag):
    """call(recipe=, tensor_format=) against its chain, its replay and its replay with the draws on the device"""
    np.random.seed(41)
    res = call(recipe=recipe)
    after = np.random.uniform()
    assert len(res) == base + 1 and isinstance(res[-1], engine.RecipeDraw), tag
    x, draw = res[0], res[-1]
    assert (draw.windows is None) == (recipe.view is None) and (draw.color is None) == (recipe.color is None), tag
    assert (draw.post is None) == (recipe.noise is None and recipe.tone is None), tag
    assert _same_bits(x.cpu(), _chain_of(full_call, recipe, draw, fmt).cpu()), tag
    np.random.seed(1)
    before = np.random.get_state()[1].copy()
    x2 = call(recipe=recipe, recipe_draw=draw)
    assert np.array_equal(np.random.get_state()[1], before), tag              # a replay draws nothing
    assert _same_bits(x2[0].cpu(), x.cpu()), tag
    d2 = x2[-1]
    if draw.post is not None:
        for a, b in zip(d2.post[1::2], draw.post[1::2]):                      # the tables and the codes
            assert (a is None and b is None) or np.array_equal(a, b), tag
    x3 = call(recipe=recipe, recipe_draw=_to_device(draw))
    assert _same_bits(x3[0].cpu(), x.cpu()), tag
    return after


@pytest.mark.parametrize("method", ["macenko", "vahadane"])
def test_recipe_through_the_batch_methods_is_the_chain_of_existing_calls(method):
    dev = _class_batch()
    n = dev.shape[0]
    nz = stainlib_amd.MacenkoNormalizer() if method == "macenko" else stainlib_amd.VahadaneNormalizer()
    nz.fit(so.synth_tile(64, 64, 1001, so.M_TRUE_TGT))
    np.random.seed(9)
    ab = stainlib_amd.StainJitter().draw(n)
    fmt = _f16()
    recipes = _recipes()
    for k, recipe in enumerate(recipes):
        f = fmt if k % 2 == 0 else None
        bg = k % 3 == 1
        _check_method(lambda **kw: nz.augment_batch(dev, ab, augment_background=bg, tensor_format=f, **kw),
                      lambda **kw: nz.augment_batch(dev, ab, augment_background=bg, **kw), recipe, f, 4, (method, "augment", k))
    for k in (0, 1, 6, 8):
        _check_method(lambda **kw: nz.transform_batch(dev, tensor_format=fmt, **kw), lambda **kw: nz.transform_batch(dev, **kw), recipes[k],
                      fmt, 4, (method, "transform", k))
        _check_method(lambda **kw: nz.augment_batch(dev, ab, normalize=False, **kw), lambda **kw: nz.augment_batch(dev, ab, normalize=False, **kw),
                      recipes[k], None, 4, (method, "own matrix", k))
    # the failed fit: the recipe on its own bytes
    res = nz.transform_batch(dev, recipe=recipes[9])
    assert int(res[3][5]) != 0 and np.array_equal(res[0][5].cpu().numpy(), hsb_reference(dev[5].cpu().numpy(), res[-1].color.codes[5]))
    # StainAugmentor: alpha_beta, then the recipe's draws
    sa = stainlib_amd.StainAugmentor(method, sigma1=0.15, sigma2=0.1)
    for k in (0, 1, 5):
        np.random.seed(43)
        ab2 = stainlib_amd.StainJitter(0.15, 0.1).draw(n)
        np.random.seed(43)
        res = sa.augment_batch(dev, recipe=recipes[k], tensor_format=fmt)
        want = _chain_of(lambda **kw: sa.augment_batch(dev, ab2, **kw), recipes[k], res[-1], fmt)
        assert len(res) == 5 and _same_bits(res[0].cpu(), want.cpu()), (method, "StainAugmentor", k)
        again = sa.augment_batch(dev, ab2, recipe=recipes[k], recipe_draw=res[-1], tensor_format=fmt)
        assert _same_bits(again[0].cpu(), res[0].cpu())


def test_convert_with_a_recipe_and_labels_through_its_view():
    dev = _class_batch()
    n = dev.shape[0]
    fmt = _f16()
    hsbaug = stainlib_amd.HsbLightColorAugmenter()
    hedaug = stainlib_amd.HedLightColorAugmenter()

    def full_call(hsb=None, hsb_sigmas=None, hed=None, hed_sigmas=None, hed_biases=None):
        if hsb is not None:
            return hsbaug.transform_batch(dev, hsb_sigmas)
        if hed is not None:
            return hedaug.transform_batch(dev, hed_sigmas, hed_biases)
        return (dev,)
    for k, recipe in enumerate(_recipes()):
        recipe = stainlib_amd.Recipe(recipe.view, hsbaug if isinstance(recipe.color, stainlib_amd.HsbColorAugmenter) else
                                     (hedaug if recipe.color is not None else None), recipe.noise, recipe.tone)
        _check_method(lambda **kw: fmt.convert(dev, **kw), full_call, recipe, fmt, 1, ("convert", k))
    # the draw order on a real call: colour, tone, noise, view
    recipe = _recipes()[0]
    np.random.seed(77)
    x, draw = fmt.convert(dev, recipe=recipe)
    after = np.random.uniform()
    np.random.seed(77)
    sg = recipe.color.randomize_batch(n)
    tp, tabs = recipe.tone.randomize_batch(n)
    ns, cd = recipe.noise.randomize_batch(n)
    win = recipe.view.draw(n, 64, 64)
    assert np.random.uniform() == after
    assert np.array_equal(draw.color.sigmas, sg) and np.array_equal(draw.post.tone_tables, tabs) and np.array_equal(draw.post.noise_codes, cd)
    assert np.array_equal(draw.windows.affine, win.affine) and np.array_equal(draw.windows.field, win.field)
    # a label plane through the recipe's view and the returned windows: the nearest element at the image's own positions
    labels = torch.from_numpy(np.random.RandomState(2).randint(0, 9, (n, 64, 64)).astype(np.int32)).cuda()
    got = recipe.view.apply(labels, draw.windows, fill=-1).cpu().numpy()
    want = np.stack([elastic_nearest(labels[t].cpu().numpy(), draw.windows.affine[t], draw.windows.field[t], recipe.view.size, recipe.view.cell, -1)
                     for t in range(n)])
    assert np.array_equal(got, want)


# ---- 5. a tile's output does not depend on its place in the batch -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_permuting_tiles_with_their_draws_permutes_the_output(kind):
    dev, routes, _ = _setup()
    perm = np.array([2, 0, 3, 1])
    pt = torch.from_numpy(perm).cuda()
    r = routes["jitter_all"]
    rp = dict(r, M_src=r["M_src"][pt].contiguous(), maxC_src=r["maxC_src"][pt].contiguous(), alpha_beta=np.asarray(r["alpha_beta"])[perm])
    for colour in ("hed", "hsb"):
        stages = dict(**_colour_args(colour), **_post_args("both"))
        sp = {k: (v[perm] if hasattr(v, "shape") else v) for k, v in stages.items()}
        a = _call(kind, dev, None, None, r, stages)
        if kind in ("affine", "elastic"):
            b = _call(kind, dev[pt].contiguous(), None, None, rp, sp, windows=_affine_rows()[perm], field=_field()[perm])
        else:
            b = _call(kind, dev[pt].contiguous(), None, None, rp, sp, windows=_tile_view(kind)[1][perm])
        assert torch.equal(b, a[pt]), (kind, colour)
