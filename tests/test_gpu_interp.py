"""Slice interpolation on the GPU (csrc/distance.hip through oct_segmentation_amd/interp.py) against the scipy restatement of tests/interp_ref.py,
which tests/test_interp.py pins to known answers.  Every comparison is integer or bit equality: there is no tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import interp_ref as R
from analysis_ref import load_fixture
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance, interp
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 130)]
WEIGHTS = [(1, 1), (1, 2), (3, 1), (0, 1), (1, 0), (32767, 1)]
FIXTURE = os.path.join(os.path.dirname(__file__), 'golden', 'pullback_demo_excerpt.npz')


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded_stack(h, w, n=3):
    """[n, h, w, 5]: densities 0.001, 0.02, 0.5 (one pixel forced into an empty draw), an empty and a full channel, as test_gpu_distance.py
    draws them.  Read-only."""
    rng = np.random.RandomState(1000 * h + w)
    st = np.zeros((n, h, w, 5), np.float32)
    for c, density in enumerate((0.001, 0.02, 0.5)):
        for i in range(n):
            m = rng.rand(h, w) < density
            if not m.any():
                m[rng.randint(h), rng.randint(w)] = True
            st[i, :, :, c] = m
    st[..., 4] = 1.0
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def ref_sd2(h, w):
    out = R.sd2_stack(seeded_stack(h, w))
    out.setflags(write=False)
    return out


# ---- 1. the signed map
@pytest.mark.parametrize('h,w', SHAPES)
def test_signed_map_equals_the_restatement_and_the_existing_maps(h, w):
    st = seeded_stack(h, w)
    d = dev(st)
    before = d.clone()
    got = interp.signed_distance_stack(d)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 5, h, w)
    assert np.array_equal(host(got), ref_sd2(h, w))
    composed = torch.where(d.permute(0, 3, 1, 2) != 0, distance.distance_stack(d, to='clear'), -distance.distance_stack(d, to='set'))
    assert torch.equal(got, composed)
    assert (got != 0).all() and (got[:, 3] == -interp.DIST_NONE).all() and (got[:, 4] == interp.DIST_NONE).all()
    one = int(L.lib().octseg_signed_distance_scratch_bytes(1, h, w, 5))
    for budget in (1, one, 2 * one + 1):                                 # one slice, one slice, two (or, at 1 x 1, all) slices per call
        assert torch.equal(interp.signed_distance_stack(d, scratch_bytes=budget), got)
    # one slice of four channels (the float4 pack) and of one channel
    assert np.array_equal(host(interp.signed_distance_stack(dev(st[1:2, :, :, 1:5]))), ref_sd2(h, w)[1:2, 1:5])
    assert np.array_equal(host(interp.signed_distance_stack(dev(st[2:3, :, :, 2:3]))), ref_sd2(h, w)[2:3, 2:3])
    assert torch.equal(d, before)                                        # the input stack is never modified


# ---- 2. the blend
@functools.lru_cache(maxsize=None)
def blend_planes_of(h, w):
    """The 15 planes of the seeded stack and the two complementary half planes as 17 slices of ONE channel (a plan blends inside a channel):
    int64 [17, 1, h, w].  Slices 3 + 5 i are empty, 4 + 5 i full, 2 + 5 i dense, 15 and 16 the halves."""
    left = np.mgrid[:h, :w][1] < (w + 1) // 2
    halves = np.stack([R.sd2_plane(left), R.sd2_plane(~left)])
    out = np.concatenate([ref_sd2(h, w).reshape(15, h, w), halves])[:, None]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize('h,w', SHAPES)
def test_blend_of_every_ordered_pair_equals_the_restatement(h, w):
    sd2 = blend_planes_of(h, w)
    k = sd2.shape[0]
    plan = np.array([(0, 0, a, b, wa, wb) for a in range(k) for b in range(k) for wa, wb in WEIGHTS], np.int32)
    plan[:, 1] = np.arange(plan.shape[0])
    m = plan.shape[0]
    want = np.stack([R.blend(sd2[a, 0], sd2[b, 0], wa, wb) for _, _, a, b, wa, wb in plan.tolist()])
    sd2_dev = torch.from_numpy(sd2.astype(np.int32)).cuda()
    out = torch.full((m, h, w, 1), 7.0, device='cuda')
    made = torch.full((m,), -3, dtype=torch.int32, device='cuda')
    assert interp.blend_planes(sd2_dev, plan, out, made) is out
    assert out.dtype == torch.float32 and np.array_equal(host(out)[..., 0], want.astype(np.float32))
    assert np.array_equal(host(made), want.reshape(m, -1).sum(axis=1)) and torch.equal(made.long(), out.sum(dim=(1, 2, 3)).long())
    # the designed pairs are among the rows: empty against full, empty and full against dense, the half-plane tie
    row = {(a, b, wa, wb): i for i, (_, _, a, b, wa, wb) in enumerate(plan.tolist())}
    res = host(out)[..., 0].astype(bool)
    assert not res[row[(3, 4, 1, 1)]].any() and res[row[(3, 4, 1, 2)]].all() and not res[row[(4, 3, 1, 2)]].any() and res[row[(4, 3, 3, 1)]].all()
    if 0 < int((sd2[2, 0] > 0).sum()) < h * w:                           # at 1 x 1 the forced pixel makes the dense plane a full one
        assert not res[row[(3, 2, 1, 2)]].any() and not res[row[(2, 3, 32767, 1)]].any()
        assert res[row[(4, 2, 1, 2)]].all() and res[row[(2, 4, 32767, 1)]].all()
    else:
        assert (h, w) == (1, 1)
    assert not res[row[(15, 16, 1, 1)]].any() and not res[row[(16, 15, 1, 1)]].any()
    assert np.array_equal(res[row[(15, 16, 3, 1)]], sd2[15, 0] > 0) and np.array_equal(res[row[(2, 7, 1, 0)]], sd2[2, 0] > 0)
    # without made
    again = torch.full((m, h, w, 1), 7.0, device='cuda')
    interp.blend_planes(sd2_dev, plan, again)
    assert torch.equal(again, out)


# ---- 3. plan handling
def guarded(shape, dtype, fill, guard=4096):
    """A contiguous CUDA view of ``shape`` inside a larger buffer filled with ``fill``; (view, whole buffer, guard elements)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * guard,), fill, dtype=dtype, device='cuda')
    return whole[guard:guard + n].view(shape), whole, guard


def guards_intact(whole, guard, fill):
    return bool((whole[:guard] == fill).all()) and bool((whole[-guard:] == fill).all())


def test_planes_not_named_stay_and_guard_bands_are_intact():
    h, w = 33, 65
    ref = ref_sd2(h, w)
    sd2, sd2_whole, g = guarded((3, 5, h, w), torch.int32, 12345)
    sd2.copy_(torch.from_numpy(ref.astype(np.int32)))
    out, out_whole, _ = guarded((4, h, w, 5), torch.float32, 7.0)
    plan = np.array([[0, 1, 0, 2, 1, 1], [2, 3, 1, 2, 2, 1], [4, 0, 0, 1, 1, 1], [3, 0, 2, 0, 5, 1], [1, 3, 2, 2, 1, 0]], np.int32)
    made, made_whole, _ = guarded((5,), torch.int32, -9)
    interp.blend_planes(sd2, plan, out, made)
    torch.cuda.synchronize()
    want = np.full((4, h, w, 5), 7.0, np.float32)
    _, want_made = R.apply_plan(ref, plan, want)
    assert np.array_equal(host(out), want) and np.array_equal(host(made), want_made)
    named = {(o, c) for c, o, *_ in plan.tolist()}
    assert all((host(out)[o, :, :, c] == 7.0).all() for o in range(4) for c in range(5) if (o, c) not in named)
    assert guards_intact(out_whole, g, 7.0) and guards_intact(sd2_whole, g, 12345) and guards_intact(made_whole, g, -9)
    assert np.array_equal(host(sd2), ref)                                # the maps are read only
    # the library clamps what the wrapper refuses: every number of a row into its range -- a wrong plane, never a stray access
    wild = np.array([[99, -5, 1000, -1000, 99999, -7], [-3, 77, -1, 2, 1 << 30, 1 << 30]], np.int32)
    clamped = np.array([[4, 0, 2, 0, 32767, 0], [0, 3, 0, 2, 32767, 32767]], np.int32)
    out.fill_(7.0)
    made.fill_(-9)
    plan_dev = torch.from_numpy(wild).cuda()
    L.check(L.lib().octseg_signed_blend(L.ptr(sd2), 3, h, w, 5, L.ptr(plan_dev), 2, L.ptr(out), 4, L.ptr(made[:2]), L.stream_ptr()))
    torch.cuda.synchronize()
    want = np.full((4, h, w, 5), 7.0, np.float32)
    _, want_made = R.apply_plan(ref, clamped, want)
    assert np.array_equal(host(out), want) and host(made).tolist() == want_made.tolist() + [-9, -9, -9]
    assert guards_intact(out_whole, g, 7.0) and guards_intact(sd2_whole, g, 12345) and guards_intact(made_whole, g, -9)
    for bad in ([[0, 1, 0, 2, 1, 1], [0, 1, 1, 2, 1, 1]], [[0, 1, 0, 2, 0, 0]], [[0, 1, 0, 3, 1, 1]], [[5, 1, 0, 2, 1, 1]], [[0, 4, 0, 2, 1, 1]],
                [[0, 1, 0, 2, 32768, 1]]):
        with pytest.raises(ValueError):
            interp.blend_planes(sd2, bad, out)
    with pytest.raises(ValueError):
        interp.blend_planes(sd2, plan, out[..., :4])
    with pytest.raises(ValueError):
        interp.blend_planes(sd2, plan, out, made[:4])
    assert (host(out) == want).all()                                     # a refused call launches nothing


# ---- 4. bridge_gaps
@functools.lru_cache(maxsize=None)
def designed_stack():
    """[6, 33, 65, 3]: channel 0 '#.#..#' (gaps of one and two), channel 1 '.#...#' (a gap at the start, a gap of three), channel 2 absent;
    reversed along the slices the gap at the start becomes one at the end.  Channel 0 holds a disc that moves and grows plus a fixed speck,
    channel 1 seeded blobs inside a moving disc; set pixels are 1 or 255."""
    h, w = 33, 65
    rng = np.random.RandomState(11)
    st = np.zeros((6, h, w, 3), np.float32)
    for i in (0, 2, 5):
        st[i, :, :, 0] = R.disc(14 + i, 24 + 3 * i, 6 + i, h, w)
        st[i, 30, 60, 0] = 1
    for i in (1, 5):
        st[i, :, :, 1] = (R.disc(16, 30 + i, 12, h, w) & (rng.rand(h, w) < 0.7)) * 255.0
    st.setflags(write=False)
    return st


@pytest.mark.parametrize('frames', [None, [2], [0], [5], [3, 4]])
@pytest.mark.parametrize('max_gap', [1, 2])
@pytest.mark.parametrize('reverse', [False, True])
def test_bridge_gaps_equals_the_reference(reverse, max_gap, frames):
    st = designed_stack()[::-1] if reverse else designed_stack()
    d = dev(st)
    before = d.clone()
    if frames is not None and len(frames) > max_gap:
        with pytest.raises(ValueError, match='max_gap'):
            interp.bridge_gaps(d, max_gap=max_gap, frames=frames)
        with pytest.raises(ValueError):
            R.bridge(st, max_gap, frames)
        return
    want, want_plan, want_made = R.bridge(st, max_gap, frames)
    got, plan, made = interp.bridge_gaps(d, max_gap=max_gap, frames=frames, return_plan=True)
    assert np.array_equal(plan, want_plan) and plan.dtype == np.int32 and np.array_equal(made, want_made)
    assert got.dtype == torch.float32 and got.data_ptr() != d.data_ptr() and np.array_equal(host(got), want)
    assert torch.equal(d, before)                                        # the input is not modified
    assert torch.equal(interp.bridge_gaps(d, max_gap=max_gap, frames=frames), got)
    if frames is None:
        assert plan.shape[0] == {1: 1, 2: 3}[max_gap] and int(made.min()) > 0 and not (plan[:, 0] == 2).any()      # something was made
        assert torch.equal(interp.bridge_gaps(d, max_gap=max_gap, scratch_bytes=1), got)      # one key slice per call
    rep = interp.bridge_report(plan, made, [f's{i}' for i in range(6)], classes=['a', 'b', 'c'])
    assert json.loads(json.dumps(rep)) == rep and sum(len(v['slice']) for v in rep.values()) == plan.shape[0]


def test_bridge_gaps_without_a_gap_and_its_refusals():
    st = designed_stack()
    d = dev(st)
    got, plan, made = interp.bridge_gaps(d, max_gap=0, return_plan=True)
    assert plan.shape == (0, 6) and made.shape == (0,) and torch.equal(got, d) and got.data_ptr() != d.data_ptr()
    for kwargs in ({'frames': [6]}, {'frames': [-1]}, {'frames': list(range(6)), 'max_gap': 6}, {'max_gap': -1}, {'max_gap': 1.5}, {'frames': [1, 2]}):
        with pytest.raises(ValueError):
            interp.bridge_gaps(d, **kwargs)
    for bad in (torch.zeros((1, 4, 4, 4), dtype=torch.float64, device='cuda'), torch.zeros((4, 4, 4), device='cuda'),
                torch.zeros((1, 0, 4, 4), device='cuda'), torch.zeros((1, 4, 4, 17), device='cuda'), torch.zeros((1, 1, 4097, 1), device='cuda')):
        for fn in (interp.signed_distance_stack, interp.bridge_gaps, lambda s: interp.resample_stack(s, 2)):
            with pytest.raises(ValueError):
                fn(bad)


# ---- 5. resample_stack
def test_resample_stack():
    st = designed_stack()
    four = np.ascontiguousarray(np.stack([st[0, :, :, 0], st[2, :, :, 0], st[5, :, :, 1], st[1, :, :, 1]])[..., None].repeat(2, axis=-1))
    four[..., 1] = four[::-1, :, :, 0]
    d = dev(four)
    before = d.clone()
    same = interp.resample_stack(d, 1)
    assert same.shape == d.shape and torch.equal(same, (d != 0).float())                      # factor 1: the identity, as 0 / 1
    want = R.resample(four, 3)
    got = interp.resample_stack(d, 3)
    assert tuple(got.shape) == (10, 33, 65, 2) and got.dtype == torch.float32 and np.array_equal(host(got), want)
    assert all(torch.equal(got[3 * i], (d[i] != 0).float()) for i in range(4))
    assert int(got[1, :, :, 0].sum()) > 0                                # something was interpolated
    for budget in (1, 3 * (int(L.lib().octseg_signed_distance_scratch_bytes(1, 33, 65, 2)) + 4 * 33 * 65 * 2)):       # windows of two and of three
        assert torch.equal(interp.resample_stack(d, 3, scratch_bytes=budget), got)
    assert np.array_equal(host(interp.resample_stack(d, 2)), R.resample(four, 2))
    single = interp.resample_stack(d[:1], 4)
    assert torch.equal(single, (d[:1] != 0).float())
    assert torch.equal(d, before)


# ---- 6. the golden excerpt
def test_golden_excerpt_bridged_equals_the_reference():
    st = load_fixture(FIXTURE)['stack']
    want, want_plan, want_made = R.bridge(st, 3)
    assert want_plan.shape[0] == 16
    d = torch.from_numpy(st).cuda().float()
    got, plan, made = interp.bridge_gaps(d, max_gap=3, return_plan=True)
    assert np.array_equal(plan, want_plan) and np.array_equal(made, want_made)
    restored = got.clone()
    for c, o, *_ in plan.tolist():
        assert np.array_equal(host(got[o, :, :, c]), want[o, :, :, c]), (o, c)
        restored[o, :, :, c] = d[o, :, :, c]
    assert torch.equal(restored, d)                                      # every other plane is the input's
    rep = interp.bridge_report(plan, made, [f'f{i:02d}' for i in range(48)])
    assert rep['Vasa vasorum']['slice'][-5:] == [27, 28, 29, 36, 37] and rep['Lumen']['slice'] == [] and rep['Lipid core']['image'] == ['f09', 'f10', 'f11']


# ---- 7. the command line
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


def test_predict_main_writes_bridge_json(cuda, tmp_path, monkeypatch):
    """``bridge=0`` (the default) changes nothing; ``bridge=2`` writes bridge.json, whose report agrees with what bridge_gaps made of the
    same stack.  The networks are untrained, so the gap is drawn into what the segmenter returns: Lumen is a disc on the first and the last
    slice (sorted order) and cleared on the middle one, the frame the network skipped."""
    from oct_segmentation_amd import predict
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(23)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first', 'm_mid']                             # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    off, zero, on = (os.path.join(tmp_path, k) for k in ('off', 'zero', 'on'))
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={zero}', 'bridge=0']) == 0
    assert _files(off) == _files(zero)
    listed = [os.path.basename(p).split('.')[0] for p in predict._image_paths(data_dir)]
    segment = predict.segment_stack
    seen = {}

    def skipping(*a, **kw):
        stack = segment(*a, **kw)
        stack[listed.index('a_first'), :, :, 0] = dev(R.disc(60, 55, 20, 120, 120))
        stack[listed.index('m_mid'), :, :, 0] = 0
        stack[listed.index('z_last'), :, :, 0] = dev(R.disc(60, 65, 30, 120, 120))
        seen['stack'] = stack.clone()
        return stack
    monkeypatch.setattr(predict, 'segment_stack', skipping)
    assert predict.main(args + [f'save_dir={on}', 'bridge=2']) == 0
    files = _files(on)
    assert sorted(files) == sorted(list(_files(off)) + ['bridge.json'])
    names = sorted(created)
    order = torch.tensor([listed.index(n) for n in names], device='cuda')
    bridged, plan, made = interp.bridge_gaps(seen['stack'][order], max_gap=2, return_plan=True)
    got = json.loads(files['bridge.json'])
    assert got == {'max_gap': 2, 'images': names, 'classes': json.loads(json.dumps(interp.bridge_report(plan, made, names)))}
    lumen = got['classes']['Lumen']
    assert lumen['slice'] == [1] and lumen['image'] == ['m_mid'] and lumen['lo'] == [0] and lumen['hi'] == [2]
    assert lumen['pixels'] == [int(bridged[1, :, :, 0].sum())] and lumen['pixels'][0] > 1256           # between the two discs' areas
    assert list(got['classes']) == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert files['m_mid_mask.png'] != _files(off)['m_mid_mask.png']       # what is rendered is the bridged stack
    for name, cols in got['classes'].items():                            # the report agrees with made, class by class
        c = CLASS_IDS[name] - 1
        assert cols['pixels'] == [int(bridged[o, :, :, c].sum()) for o in cols['slice']]
    with pytest.raises(ValueError, match='bridge'):
        predict.main(args + [f'save_dir={on}', 'bridge=-1'])
