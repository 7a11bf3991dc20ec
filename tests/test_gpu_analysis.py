"""The measurement kernels (csrc/measure.hip through oct_segmentation_amd/analysis.py and predict.py) against the numpy restatement
(tests/analysis_ref.py) and against what the reference's own get_analysis / calculate_object_thickness returned on an excerpt of its demo
pullback (tests/golden/pullback_demo_excerpt.npz).  Everything is integer, and the host arithmetic is the same float64 operations on the
same integers: every comparison is equality."""
import base64
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import analysis_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import analysis
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'pullback_demo_excerpt.npz')


def _blobs(rng, h, w, p, smooth):
    if h * w < 36:
        return rng.random((h, w)) < p
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1))
    return s > np.quantile(s, 1 - p)


def _gpu(cuda, masks):
    counts, radii = analysis.measure_stack(torch.from_numpy(np.ascontiguousarray(masks, np.float32)).to(cuda))
    n, _, _, c = masks.shape
    assert counts.dtype == radii.dtype == torch.int32 and tuple(counts.shape) == (n, c) and tuple(radii.shape) == (n, c, 360)
    return counts.cpu(), radii.cpu()


def _same(got, want, what):
    for g, w, name in zip(got, want, ('counts', 'radii')):
        w = torch.from_numpy(w)
        if not torch.equal(g, w):
            bad = torch.nonzero(g != w)
            raise AssertionError((what, name, len(bad), bad[:5].tolist(), g[g != w][:5].tolist(), w[g != w][:5].tolist()))


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 4), (17, 33), (31, 31), (64, 48), (97, 130), (130, 97)])
@pytest.mark.parametrize('n', [1, 3])
def test_kernel_equals_restatement(cuda, n, h, w):
    """Random blobs; one reference per shape, its channels reused for the 1-, 4- and 5-channel stacks (dword path, 16-byte path, dword path)
    and for a 4-channel view that starts 4 bytes into its storage (the unaligned path)."""
    rng = np.random.default_rng(7000 * h + 10 * w + n)
    masks = np.stack([np.stack([_blobs(rng, h, w, (0.15, 0.4, 0.7, 0.3, 0.55)[c], 1 + (c & 1)) for c in range(5)], axis=-1)
                      for _ in range(n)]).astype(np.float32)
    masks[masks != 0] = rng.choice(np.array([1.0, 255.0, -2.5, 1e-30], np.float32), size=int((masks != 0).sum()))   # any value != 0 is set
    want = R.measure(masks)
    for sc in (1, 4, 5):
        _same(_gpu(cuda, masks[..., :sc]), (want[0][:, :sc], want[1][:, :sc]), (n, h, w, sc))
    m4 = np.ascontiguousarray(masks[..., :4])
    buf = torch.zeros(m4.size + 8, dtype=torch.float32, device=cuda)
    buf[1:1 + m4.size] = torch.from_numpy(m4).to(cuda).flatten()
    view = buf[1:1 + m4.size].view(n, h, w, 4)
    assert view.data_ptr() % 16 == 4
    counts, radii = analysis.measure_stack(view)
    _same((counts.cpu(), radii.cpu()), (want[0][:, :4], want[1][:, :4]), (n, h, w, 'unaligned'))


def _disk(h, w, r0, r1):
    """Pixels whose distance from the walk's centre (w // 2, h // 2) lies in [r0, r1]."""
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy - h // 2) ** 2 + (xx - w // 2) ** 2
    return (d2 >= r0 * r0) & (d2 <= r1 * r1)


@pytest.mark.parametrize('h,w', [(65, 65), (140, 200)])
def test_designed_rays(cuda, h, w):
    cy, cx = h // 2, w // 2
    length = R.ray_lengths(h, w)
    assert length[0] > 30
    m = np.zeros((7, h, w, 4), np.float32)
    m[1] = 1                                                    # full frame: every ray runs to its end
    m[2, cy, cx + 1, 0] = 1                                     # a single pixel next to the centre
    m[2, cy, cx, 1] = 1                                         # the centre pixel alone: angle 0 steps over it (step 1 is already cx + 1)
    m[3, :, :, 0] = _disk(h, w, 10, 15)                         # a ring: the gap before the object is skipped
    m[3, :, :, 1] = _disk(h, w, 10, 15) | _disk(h, w, 20, 25)   # two concentric rings: only the first counts
    m[3, :, :, 2] = _disk(h, w, 0, 15)                          # the same outer edge, from the centre on
    m[4, cy - 2:cy + 3, cx + 3:, 0] = 1                         # touches the right border
    m[4, :cy - 5, cx - 2:cx + 3, 1] = 1                         # touches the top border (angle 270)
    m[4, 0, :, 2] = 1; m[4, h - 1, :, 2] = 1; m[4, :, 0, 2] = 1; m[4, :, w - 1, 2] = 1     # the frame's outline
    m[5, :, :, 0] = _disk(h, w, 0, 5)                           # four classes resolving at different steps of the same angle
    m[5, :, :, 1] = _disk(h, w, 0, 20)
    m[5, :, :, 2] = _disk(h, w, 25, 30)
    m[5, cy, cx + 2:cx + 4, 3] = 1
    m[6, :, :, 1] = _disk(h, w, 3, 4)                           # only one class has anything
    counts, radii = _gpu(cuda, m)
    _same((counts, radii), R.measure(m), (h, w))
    radii, counts = radii.numpy(), counts.numpy()
    assert not radii[0].any() and not counts[0].any()
    assert (radii[1] == length[None, :]).all() and (counts[1] == h * w).all()
    assert radii[2, 0, 0] == 1 and counts[2, 0] == 1
    assert radii[2, 1, 0] == 0 and radii[2, 1, 45] == 1 and counts[2, 1] == 1      # int(c + cos 45) = c: other angles do sample the centre
    for a in (0, 90, 180):                                      # (at 270 degrees cos is -1.8e-16 and the ray runs along column cx - 1)
        assert radii[3, 0, a] == radii[3, 1, a] == radii[3, 2, a] == 15, a
    assert (radii[3, 0] == radii[3, 1]).all() and (radii[3, 0] > 0).all()
    assert radii[4, 0, 0] == length[0] == w - cx - 1 and radii[4, 1, 270] == length[270] == cy
    assert list(radii[5, :, 0]) == [5, 20, 30, 3]
    assert not radii[6, 0].any() and radii[6, 1].any() and not radii[6, 2:].any()


def test_chunk_seams_of_the_64_lane_walk(cuda):
    """An object along angle 0 that starts at step 63, 64 or 65 and ends at step 127, 128 or 129: the seams between the 64-step chunks.
    The 40 x 300 frame gives angle 0 a ray of 149 steps."""
    h, w = 40, 300
    cy, cx = h // 2, w // 2
    length = R.ray_lengths(h, w)
    assert length[0] == 149
    cases = [(s, e) for s in (63, 64, 65) for e in (127, 128, 129)]
    m = np.zeros((len(cases), h, w, 4), np.float32)
    for i, (s, e) in enumerate(cases):
        m[i, cy, cx + s:cx + e + 1, 0] = 1                      # steps s..e
        m[i, cy, cx + s:, 1] = 1                                # from step s to the border
        m[i, cy, cx + 1:cx + e + 1, 2] = 1                      # from step 1 to step e
        m[i, cy, cx + e, 3] = 1; m[i, cy, cx + e + 2, 3] = 1    # one step, a gap, another object
    counts, radii = _gpu(cuda, m)
    _same((counts, radii), R.measure(m), 'seams')
    for i, (s, e) in enumerate(cases):
        assert list(radii[i, :, 0]) == [e, 149, e, e], (s, e)


def test_fixture_equals_the_references_get_analysis(cuda):
    fx = R.load_fixture(FIXTURE)
    rec = fx['recorded']
    stack = torch.from_numpy(fx['stack']).to(cuda).to(torch.float32)
    assert tuple(stack.shape) == (48, 750, 750, 4)
    data = analysis.analyze_stack(stack, fx['names'])
    assert data['ratio'] == rec['ratio'] and data['images'] == rec['images'] and list(data['objects']) == list(rec['objects'])
    for cl, want in rec['objects'].items():
        got = data['objects'][cl]
        for k in ('slice', 'area', 'object_id', 'img_name'):
            assert got[k] == want[k], (cl, k)
        assert got['masks'] == []
        ch = CLASS_IDS[cl] - 1
        assert got['thickness_mean'] == [fx['thickness'][(s, ch)]['median'] / rec['ratio'] for s in want['slice']], cl
        assert got['thickness_min'] == [fx['thickness'][(s, ch)]['min'] / rec['ratio'] for s in want['slice']], cl
        assert got['thickness_max'] == [fx['thickness'][(s, ch)]['max'] / rec['ratio'] for s in want['slice']], cl
    counts, radii = analysis.measure_stack(stack)
    radii = radii.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), fx['stack'].reshape(48, -1, 4).sum(axis=1))
    for (s, c), want in fx['thickness'].items():
        assert analysis.radial_thickness(radii[s, c]) == want, (s, c)
    assert json.loads(json.dumps(data)) == data


def test_with_masks_round_trips(cuda):
    rng = np.random.default_rng(3)
    n, h, w = 3, 20, 24
    masks = np.stack([np.stack([_blobs(rng, h, w, 0.4, 1) for _ in range(4)], axis=-1) for _ in range(n)]).astype(np.float32)
    masks[1, :, :, 2] = 0                                       # an absent class
    masks[2, :, :, 0] = 1                                       # a full mask: absent by upstream's rule
    stack = torch.from_numpy(masks).to(cuda)
    plain = analysis.analyze_stack(stack)
    data = analysis.analyze_stack(stack, with_masks=True)
    assert plain['images'] == ['0', '1', '2'] and plain['ratio'] == 3
    assert plain['objects']['Lumen']['slice'] == [0, 1] and plain['objects']['Lipid core']['slice'] == [0, 2]
    for cl, obj in data['objects'].items():
        assert [v for k, v in obj.items() if k != 'masks'] == [v for k, v in plain['objects'][cl].items() if k != 'masks']
        assert plain['objects'][cl]['masks'] == [] and len(obj['masks']) == len(obj['slice'])
        for s, b64 in zip(obj['slice'], obj['masks']):
            img = Image.open(io.BytesIO(base64.b64decode(b64)))
            assert img.mode == 'L'
            assert np.array_equal(np.asarray(img), (masks[s, :, :, CLASS_IDS[cl] - 1] * 255).astype(np.uint8))
    json.dumps(data)
    want = analysis.build_analysis(*R.measure(masks), h, w, ['0', '1', '2'])
    assert plain == want


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


def test_predict_main_writes_analysis_json(cuda, tmp_path):
    from oct_segmentation_amd import predict
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(13)
    data_dir, save = os.path.join(tmp_path, 'input'), os.path.join(tmp_path, 'output')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first', 'm_mid']                    # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', f'save_dir={save}', 'output_size=[120,120]', 'compute_dtype=fp32']
    assert predict.main(args + ['analysis=true']) == 0
    assert sorted(os.listdir(save)) == sorted(['analysis.json'] + [f'{n}_{k}.png' for n in created for k in ('mask', 'overlay')])
    with open(os.path.join(save, 'analysis.json')) as f:
        got = json.load(f)
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    want = analysis.analyze_stack(stack, names)
    assert got['images'] == names and got['ratio'] == 18
    assert got == json.loads(json.dumps(want))
    # without the key nothing of the kind is written
    save2 = os.path.join(tmp_path, 'output2')
    assert predict.main([f'data_dir={os.path.join(data_dir, "a_first.png")}', f'models_dir={models}', f'save_dir={save2}', 'output_size=[64,64]',
                         'compute_dtype=fp32', 'classes=[Lumen]']) == 0
    assert sorted(os.listdir(save2)) == ['a_first_mask.png', 'a_first_overlay.png']


def test_abi_refuses_bad_arguments(cuda):
    lib = L.lib()
    h, w = 8, 8
    pix_np, len_np = analysis.ray_table(h, w)
    R_ = pix_np.shape[1]
    s = torch.ones((1, h, w, 4), dtype=torch.float32, device=cuda)
    pix, length = torch.from_numpy(pix_np).to(cuda), torch.from_numpy(len_np).to(cuda)
    counts = torch.full((1, 17), 9, dtype=torch.int32, device=cuda)
    radii = torch.full((1, 17, 360), 9, dtype=torch.int32, device=cuda)
    st, p = L.stream_ptr(), L.ptr
    BAD_SHAPE, BAD_ARG = -1, -5

    def call(stack=s, N=1, H=h, W=w, SC=4, rp=pix, rl=length, R=R_, c=counts, r=radii):
        return lib.octseg_stack_measure(p(stack), N, H, W, SC, p(rp), p(rl), R, p(c), p(r), st)

    for kw in ({'stack': None}, {'rp': None}, {'rl': None}, {'c': None}, {'r': None}):
        assert call(**kw) == BAD_ARG, kw
        assert b'null' in lib.octseg_last_error()
    for kw in ({'N': 0}, {'N': -1}, {'H': 0}, {'W': -1}, {'SC': 0}, {'SC': 17}, {'R': -1}, {'H': 65536, 'W': 32768}):
        assert call(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert (counts == 9).all() and (radii == 9).all()          # nothing was launched
    # a null table is fine when there are no steps; a 1 x 1 frame has none
    one = torch.ones((2, 1, 1, 4), dtype=torch.float32, device=cuda)
    assert call(stack=one, N=2, H=1, W=1, rp=None, R=0) == 0
    torch.cuda.synchronize()
    assert (counts.flatten()[:8] == 1).all() and (radii.flatten()[:2 * 4 * 360] == 0).all() and (radii.flatten()[2 * 4 * 360:] == 9).all()
    # table entries outside the frame and lengths outside [0, R] are clamped on the device, not followed
    wild = pix.clone()
    wild[0, :] = torch.tensor([-5, 2 ** 31 - 1, 10 ** 6][:R_] + [0] * max(R_ - 3, 0), dtype=torch.int32, device=cuda)[:R_]
    long_len = length.clone()
    long_len[0] = 10 ** 6; long_len[1] = -7
    assert call(rp=wild, rl=long_len, SC=4) == 0
    torch.cuda.synchronize()
    got = radii[0, :4].cpu()
    assert (got[:, 0] == R_).all() and (got[:, 1] == 0).all() and (got[:, 2:] == torch.from_numpy(len_np)[2:]).all()
    # the Python wrapper refuses what the kernel cannot take
    for bad in (s.double(), s[0], s.cpu(), s[:0], torch.ones((1, 2, 2, 17), dtype=torch.float32, device=cuda)):
        with pytest.raises(ValueError):
            analysis.measure_stack(bad)
