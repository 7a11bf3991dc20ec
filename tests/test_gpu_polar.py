"""csrc/polar.hip on the GPU against the numpy restatement (tests/polar_ref.py): exact integer equality everywhere.  Every case also holds the
invariants of the profile, among them OUT == measure_stack's radii: that kernel is independent and itself pinned to the reference's values."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import analysis_ref as R
import polar_ref as P
from oct_segmentation_amd import analysis, cleanup, polar
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'pullback_demo_excerpt.npz')
IN, OUT, LAST, HITS, RUNS = range(5)


def _blobs(rng, h, w, p, smooth):
    if h * w < 36:
        return rng.random((h, w)) < p
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1))
    return s > np.quantile(s, 1 - p)


def _diff(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[got != want][:5].tolist(), want[got != want][:5].tolist()))


def _run(stack):
    """stack: float32 CUDA [N, H, W, SC].  Runs the kernel with and without the map, checks shapes, that the two profiles agree, and every
    invariant; returns (prof, map) as numpy."""
    n, h, w, sc = (int(v) for v in stack.shape)
    width = P.table_width(h, w)
    plain = polar.polar_profile(stack)
    prof, labels = polar.polar_profile(stack, want_map=True)
    _, radii = analysis.measure_stack(stack)
    assert prof.dtype == plain.dtype == torch.int32 and tuple(prof.shape) == tuple(plain.shape) == (n, sc, 360, 5)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n, 360, width)
    prof, plain, labels, radii = prof.cpu().numpy(), plain.cpu().numpy(), labels.cpu().numpy(), radii.cpu().numpy()
    _diff(plain, prof, 'with and without the map')
    _diff(prof[..., OUT], radii, 'OUT against measure_stack')
    length = R.ray_lengths(h, w)[None, None, :]
    met = prof[..., IN] > 0
    assert (prof >= 0).all()
    assert (prof[..., IN] <= prof[..., OUT]).all() and (prof[..., OUT] <= prof[..., LAST]).all() and (prof[..., LAST] <= length).all()
    assert (prof[..., OUT] >= 1)[met].all() and not prof[~met].any()
    assert (prof[..., HITS] >= prof[..., OUT] - prof[..., IN] + 1)[met].all()
    assert ((prof[..., RUNS] >= 1) == met).all()
    for c in range(sc):
        _diff(prof[:, c, :, HITS], ((labels >> c) & 1).sum(axis=2), ('HITS against the popcount of bit plane', c))
    assert not (labels >> sc).any() if sc < 8 else True
    return prof, labels


def _dev(cuda, masks):
    return torch.from_numpy(np.ascontiguousarray(masks, np.float32)).to(cuda)


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 4), (17, 33), (64, 48), (97, 130), (130, 97)])
@pytest.mark.parametrize('n', [1, 3])
def test_kernel_equals_restatement(cuda, n, h, w):
    """Random blobs; one reference per shape over eight channels, its channels reused for the 1-, 4-, 5- and 8-channel stacks (dword path,
    16-byte path, dword paths) and for a 4-channel view that starts 4 bytes into its storage (the unaligned path).  97 x 130 and 130 x 97 have
    rays of 48 to 80 steps: about half of them cross one chunk seam."""
    rng = np.random.default_rng(9000 * h + 10 * w + n)
    ps = (0.15, 0.4, 0.7, 0.3, 0.55, 0.05, 0.9, 0.25)
    masks = np.stack([np.stack([_blobs(rng, h, w, ps[c], 1 + (c & 1)) for c in range(8)], axis=-1) for _ in range(n)]).astype(np.float32)
    masks[masks != 0] = rng.choice(np.array([1.0, 255.0, -2.5, 1e-30], np.float32), size=int((masks != 0).sum()))   # any value != 0 is set
    want, want_map = P.profile(masks)
    if h * w == 97 * 130:
        length = R.ray_lengths(h, w)
        assert length.min() < 64 and (length > 64).sum() > 100 and length.max() == 80
    for sc in (1, 4, 5, 8):
        prof, labels = _run(_dev(cuda, masks[..., :sc]))
        _diff(prof, want[:, :sc], (n, h, w, sc, 'prof'))
        _diff(labels, want_map & ((1 << sc) - 1), (n, h, w, sc, 'map'))
    m4 = np.ascontiguousarray(masks[..., :4])
    buf = torch.zeros(m4.size + 8, dtype=torch.float32, device=cuda)
    buf[1:1 + m4.size] = torch.from_numpy(m4).to(cuda).flatten()
    view = buf[1:1 + m4.size].view(n, h, w, 4)
    assert view.data_ptr() % 16 == 4
    prof, labels = _run(view)
    _diff(prof, want[:, :4], (n, h, w, 'unaligned', 'prof'))
    _diff(labels, want_map & 15, (n, h, w, 'unaligned', 'map'))
    if (h, w) == (1, 1):
        assert not prof.any() and labels.shape == (n, 360, 0)


def test_chunk_seams_of_the_64_lane_walk(cuda):
    """Patterns along angle 0 of a 40 x 300 frame (149 steps: chunks of 64, 64 and 21) that sit on, straddle and alternate across the seams."""
    h, w = 40, 300
    cy, cx = h // 2, w // 2
    assert R.ray_lengths(h, w)[0] == 149
    patterns = [([64], (64, 64, 64, 1, 1)), ([65], (65, 65, 65, 1, 1)), ([128], (128, 128, 128, 1, 1)), ([129], (129, 129, 129, 1, 1)),
                (list(range(60, 65)) + list(range(66, 71)), (60, 64, 70, 10, 2)),
                (list(range(1, 65)), (1, 64, 64, 64, 1)), (list(range(65, 150)), (65, 149, 149, 85, 1)),
                (list(range(1, 150)), (1, 149, 149, 149, 1)),
                (list(range(1, 150, 2)), (1, 1, 149, 75, 75)), (list(range(2, 150, 2)), (2, 2, 148, 74, 74)),
                (list(range(1, 150, 3)), (1, 1, 148, 50, 50)), (list(range(3, 150, 3)), (3, 3, 147, 49, 49)),
                (list(range(2, 150, 3)) + list(range(3, 150, 3)), (2, 3, 149, 99, 50)),
                (list(range(140, 150)), (140, 149, 149, 10, 1)), ([63, 64, 65, 127, 128, 129], (63, 65, 129, 6, 2)),
                ([64, 128], (64, 64, 128, 2, 2)), ([1, 149], (1, 1, 149, 2, 2))]
    while len(patterns) % 4:
        patterns.append(([], (0, 0, 0, 0, 0)))
    m = np.zeros((len(patterns) // 4, h, w, 4), np.float32)
    for i, (steps, _) in enumerate(patterns):
        for r in steps:
            m[i // 4, cy, cx + r, i % 4] = 1                   # angle 0: step r is pixel (cy, cx + r)
    prof, labels = _run(_dev(cuda, m))
    want, want_map = P.profile(m)
    _diff(prof, want, 'seams prof')
    _diff(labels, want_map, 'seams map')
    for i, (steps, fields) in enumerate(patterns):
        assert tuple(prof[i // 4, i % 4, 0]) == fields, (i, steps[:4], tuple(prof[i // 4, i % 4, 0]), fields)


def _disk(h, w, r0, r1):
    """Pixels whose distance from the walk's centre (w // 2, h // 2) lies in [r0, r1]."""
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy - h // 2) ** 2 + (xx - w // 2) ** 2
    return (d2 >= r0 * r0) & (d2 <= r1 * r1)


@pytest.mark.parametrize('h,w', [(65, 65), (140, 200)])
def test_designed_frames(cuda, h, w):
    cx = w // 2
    length = R.ray_lengths(h, w)
    m = np.zeros((6, h, w, 4), np.float32)
    m[1] = 1                                                    # full frame; slice 0 stays empty
    m[2, :, cx + 1:, 0] = 1                                     # the right half-plane, from step 1 of angle 0 on
    m[2, :, :, 1] = _disk(h, w, 10, 15)                         # a full ring
    m[2, :, :, 2] = _disk(h, w, 10, 15) | _disk(h, w, 20, 25)   # two concentric rings
    cap, right = _disk(h, w, 8, 12), np.zeros((h, w), bool)
    right[:, cx + 6:] = True
    m[3, :, :, 1] = cap                                         # a cap ring ...
    m[3, :, :, 2] = _disk(h, w, 18, 24) & right                 # ... with lipid behind it on the right side only
    m[4, :, :, 1] = _disk(h, w, 18, 24)                         # lipid in FRONT of the cap: nothing lies behind the cap
    m[4, :, :, 2] = _disk(h, w, 8, 12) & right
    m[5, :, :, 1] = cap                                         # lipid that starts inside the cap's run and ends with it: not behind it
    m[5, :, :, 2] = _disk(h, w, 10, 12)
    prof, labels = _run(_dev(cuda, m))
    want, want_map = P.profile(m)
    _diff(prof, want, (h, w, 'prof'))
    _diff(labels, want_map, (h, w, 'map'))
    assert not prof[0].any() and not labels[0].any()
    for c in range(4):                                          # IN = 1, OUT = LAST = HITS = len, RUNS = 1
        assert (prof[1, c] == np.stack([np.ones_like(length), length, length, length, np.ones_like(length)], axis=1)).all()
    assert (labels[1] == np.where(np.arange(labels.shape[2])[None, :] < length[:, None], 15, 0)).all()
    s = polar.summarize(prof)
    for n in range(6):
        for c in range(4):
            ref = P.summary(prof[n, c])
            assert {k: s[k][n, c] for k in ref} == ref, (n, c)
    # the right half-plane: cos > 0 on 271 .. 359 and 0 .. 89, so the arc wraps through 0 and starts above 180
    assert prof[2, 0, 0, IN] == 1 and prof[2, 0, 180, IN] == 0
    assert 170 <= s['arc'][2, 0] <= 181 and s['arc_max'][2, 0] == s['arc'][2, 0] and 268 <= s['arc_start'][2, 0] <= 275
    assert (s['arc'][2, 1], s['arc_max'][2, 1], s['arc_start'][2, 1]) == (360, 360, 0)
    assert (prof[2, 2, :, RUNS] == 2).all() and (prof[2, 2, :, LAST] >= 20).all() and (prof[2, 2, :, OUT] <= 16).all()
    assert (prof[2, 2, :, :2] == prof[2, 1, :, :2]).all()      # IN and OUT are those of the inner ring alone
    for a in (0, 90, 180):
        assert tuple(prof[2, 2, a]) == (10, 15, 25, 12, 2), a
    o = polar.overlap(prof, 1, 2)
    for n in range(6):
        ref = P.cover(prof[n, 1], prof[n, 2])
        assert {k: o[k][n] for k in ref} == ref, n
    # cap with lipid behind it on one side: the overlap is the lipid's arc, through 0
    assert s['arc'][3, 1] == 360 and 0 < s['arc'][3, 2] < 180
    assert (o['arc'][3], o['arc_max'][3], o['arc_start'][3]) == (s['arc'][3, 2], s['arc_max'][3, 2], s['arc_start'][3, 2])
    assert o['arc_start'][3] > 180 and 3 <= o['cover_min'][3] <= 6 and o['cover_argmin'][3] >= 0
    assert (o['arc'][4], o['arc_max'][4], o['arc_start'][4], o['cover_min'][4], o['cover_argmin'][4]) == (0, 0, -1, 0, -1)
    assert o['arc'][5] == 0 and polar.overlap(prof, 2, 1)['arc'][4] == s['arc'][4, 2] > 0


def test_demo_excerpt_equals_restatement(cuda):
    """Slices 0, 1, 8 and 12 of the demo excerpt hold cap and lipid, slice 2 neither; 750 x 750, rays of up to 529 steps."""
    fx = R.load_fixture(FIXTURE)
    pick = [0, 1, 8, 12, 2]
    masks = fx['stack'][pick]
    prof, labels = _run(_dev(cuda, masks))
    want, want_map = P.profile(masks)
    _diff(prof, want, 'demo prof')
    _diff(labels, want_map, 'demo map')
    s, o = polar.summarize(prof), polar.overlap(prof, 1, 2)
    assert (s['arc'][:4, 1:3] > 0).all() and (s['arc'][4, 1:3] == 0).all() and o['arc'][4] == 0
    # slice 0, restated on the host when this was planned: lipid arc 130, cap met on 127, cap over lipid on 118 with a thinnest cap of 21 steps
    assert (s['arc'][0, 2], s['arc'][0, 1], o['arc'][0], o['cover_min'][0]) == (130, 127, 118, 21)
    rep = polar.plaque_report(_dev(cuda, masks), [fx['names'][i] for i in pick])
    assert rep['ratio'] == 112 and rep['classes']['Lipid core']['slice'] == [0, 1, 2, 3] and rep['cap_over_lipid']['slice'][0] == 0
    assert rep['cap_over_lipid']['cap_min'][0] == 21 / 112 and rep['classes']['Lipid core']['arc'][0] == 130
    assert rep == polar.build_report(want, 750, [fx['names'][i] for i in pick])
    assert json.loads(json.dumps(rep)) == rep


@pytest.mark.parametrize('c', [1, 3])
def test_unwrap_equals_fancy_indexing(cuda, c):
    rng = np.random.default_rng(50 + c)
    for n, h, w in ((2, 1, 1), (1, 5, 4), (3, 97, 130), (2, 40, 300)):
        frames = rng.integers(1, 256, (n, h, w, c), dtype=np.uint8)        # no zeros: a zero in the output is past the ray's end
        got = polar.unwrap_frames(torch.from_numpy(frames).to(cuda))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 360, P.table_width(h, w), c)
        got = got.cpu().numpy()
        _diff(got, P.unwrap(frames), (n, h, w, c))
        length = R.ray_lengths(h, w)
        past = np.arange(got.shape[2])[None, :] >= length[:, None]
        assert not got[:, past].any() and got[:, ~past].all()


def test_abi_on_the_device(cuda):
    """Refusals leave device buffers untouched; a null table is fine without steps; wild table entries and lengths are clamped, not followed."""
    from oct_segmentation_amd import _lib as L
    lib = L.lib()
    h, w = 8, 8
    pix_np, len_np = analysis.ray_table(h, w)
    width = pix_np.shape[1]
    s = torch.ones((1, h, w, 4), dtype=torch.float32, device=cuda)
    pix, length = torch.from_numpy(pix_np).to(cuda), torch.from_numpy(len_np).to(cuda)
    prof = torch.full((2 * 9 * 360 * 5,), 9, dtype=torch.int32, device=cuda)
    labels = torch.full((2 * 360 * width + 16,), 9, dtype=torch.uint8, device=cuda)
    st, p = L.stream_ptr(), L.ptr

    def call(stack=s, N=1, H=h, W=w, SC=4, rp=pix, rl=length, R_=width, pr=prof, mp=labels):
        return lib.octseg_stack_polar(p(stack), N, H, W, SC, p(rp), p(rl), R_, p(pr), p(mp), st)

    for kw in ({'stack': None}, {'rp': None}, {'rl': None}, {'pr': None}, {'N': 0}, {'H': 0}, {'W': -1}, {'SC': 0}, {'SC': 9}, {'R_': -1},
               {'H': 65536, 'W': 32768}):
        assert call(**kw) == -5, kw
    torch.cuda.synchronize()
    assert (prof == 9).all() and (labels == 9).all()           # nothing was launched
    one = torch.ones((2, 1, 1, 4), dtype=torch.float32, device=cuda)
    assert call(stack=one, N=2, H=1, W=1, rp=None, R_=0) == 0   # a 1 x 1 frame has no steps: zero profiles, no map entry
    torch.cuda.synchronize()
    assert (prof[:2 * 4 * 360 * 5] == 0).all() and (prof[2 * 4 * 360 * 5:] == 9).all() and (labels == 9).all()
    wild = pix.clone()
    wild[0, :3] = torch.tensor([-5, 2 ** 31 - 1, 10 ** 6], dtype=torch.int32, device=cuda)
    long_len = length.clone()
    long_len[0] = 10 ** 6; long_len[1] = -7
    assert call(rp=wild, rl=long_len) == 0
    torch.cuda.synchronize()
    got = prof[:4 * 360 * 5].view(4, 360, 5).cpu().numpy()
    got_map = labels[:360 * width].view(360, width).cpu().numpy()
    assert (got[:, 0] == (1, width, width, width, 1)).all()     # the length is clamped to the table's width, every sample is a frame pixel
    assert not got[:, 1].any()                                  # a negative length is an empty ray
    assert (got_map[0] == 15).all() and not got_map[1].any() and (labels[360 * width:] == 9).all()
    assert (got[:, 2:, 1] == len_np[None, 2:]).all()


def test_report_with_clean_and_analyze_stack_unchanged(cuda):
    rng = np.random.default_rng(5)
    n, h, w = 2, 60, 64
    masks = np.stack([np.stack([_blobs(rng, h, w, 0.35, 2) for _ in range(4)], axis=-1) for _ in range(n)]).astype(np.float32)
    stack = _dev(cuda, masks)
    before = analysis.analyze_stack(stack)
    rep = polar.plaque_report(stack, clean=True)
    cleaned = cleanup.clean_stack(stack)
    assert not torch.equal(cleaned, stack)
    assert rep == polar.plaque_report(cleaned) and rep != polar.plaque_report(stack)
    assert rep == polar.plaque_report(stack, clean={}) and rep['images'] == ['0', '1'] and rep['ratio'] == 9
    assert rep == polar.build_report(P.profile(cleaned.cpu().numpy())[0], h)
    assert torch.equal(stack, _dev(cuda, masks)) and analysis.analyze_stack(stack) == before      # the input is not written
    with pytest.raises(ValueError, match='ratio'):
        polar.plaque_report(torch.ones((1, 5, 5, 4), device=cuda))
    carpet = polar.carpet_view(polar.polar_profile(stack), list(CLASS_IDS))
    assert carpet.shape == (360, n, 3) and carpet.dtype == np.uint8


def _models_dir(cuda, root):
    from oct_segmentation_amd.model import OCTSegmentationModel
    specs = {'LM': ('unet', ['Lumen'], 64), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap'], 96), 'VV': ('unet', ['Vasa vasorum'], 64)}
    for d, (arch, classes, size) in specs.items():
        os.makedirs(os.path.join(root, d))
        m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=len(d) + 3, compute_dtype=torch.float32)
        m.save_checkpoint(os.path.join(root, d, 'weights.ckpt'))
        with open(os.path.join(root, d, 'config.json'), 'w') as f:
            json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': size, 'classes': classes}, f)
    return root


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), 'rb') as f:
            out[name] = f.read()
    return out


def test_predict_main_writes_plaque_files(cuda, tmp_path):
    """Both input kinds: a directory of files (sorted file-name order, as analysis=true) and a .npy volume (analyze_pullback)."""
    from oct_segmentation_amd import predict, pullback
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(17)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first', 'm_mid']                    # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true']
    off, on = os.path.join(tmp_path, 'off'), os.path.join(tmp_path, 'on')
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={on}', 'plaque=true']) == 0
    a, b = _files(off), _files(on)
    assert sorted(b) == sorted(list(a) + ['plaque.json', 'plaque_carpet.png']) and 'analysis.json' in a
    for name in a:                                              # analysis.json, overlays and colour masks do not change
        assert a[name] == b[name], name
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    want = polar.plaque_report(stack, names)
    got = json.loads(b['plaque.json'])
    assert got == json.loads(json.dumps(want)) and got['images'] == names and got['ratio'] == 18
    assert any(len(o['slice']) for o in got['classes'].values())               # the nets found something to profile
    carpet = np.asarray(Image.open(os.path.join(on, 'plaque_carpet.png')))
    assert np.array_equal(carpet, polar.carpet_view(polar.polar_profile(stack), list(CLASS_IDS))) and carpet.shape == (360, 3, 3)
    # the volume path
    vol = rng.integers(0, 256, (2, 90, 90, 3), dtype=np.uint8)
    np.save(os.path.join(tmp_path, 'pull.npy'), vol)
    vargs = [f'data_dir={os.path.join(tmp_path, "pull.npy")}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true']
    voff, von = os.path.join(tmp_path, 'voff'), os.path.join(tmp_path, 'von')
    assert predict.main(vargs + [f'save_dir={voff}']) == 0
    assert predict.main(vargs + [f'save_dir={von}', 'plaque=true']) == 0
    a, b = _files(voff), _files(von)
    assert sorted(b) == sorted(list(a) + ['plaque.json', 'plaque_carpet.png']) and len(a) == 5
    for name in a:
        assert a[name] == b[name], name
    res = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32,
                                    plaque=True)
    assert res.plaque == polar.plaque_report(res.stack, ['pull_001', 'pull_002'], ratio=13) and res.plaque['ratio'] == 13
    assert json.loads(b['plaque.json']) == json.loads(json.dumps(res.plaque))
    wide = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), compute_dtype=torch.float32,
                                     plaque={'wide_arc': 10, 'thin_cap': 5.0}, clean=True)
    assert wide.plaque == polar.plaque_report(wide.stack, ['001', '002'], ratio=13, wide_arc=10, thin_cap=5.0)
    for bad in ({'bogus': 1}, 'yes'):                           # refused before any work
        with pytest.raises(ValueError, match='plaque'):
            pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), compute_dtype=torch.float32, plaque=bad)
