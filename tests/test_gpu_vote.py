"""The voted serving epilogue on the GPU: octseg_vote_assemble against tests/vote_ref.py on every case of tests/vote_cases.py (EVERY pixel: the CPU
test pins that no case has a soft near-tie), the view algebra through the kernel, the one-member launch against octseg_mask_assemble, and
segment_stack_voted / predict.main end to end on small networks."""
import json
import os

import numpy as np
import pytest
import torch

import vote_cases as VC
import vote_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import vote

pytestmark = pytest.mark.gpu
MODE_NAMES = ('soft', 'majority')
FILL = 7.0            # what the untouched channels of the outputs hold


def _run(cuda, members, channels, views, N, oh, ow, mode, rows=None, cols=None, prob=True, dissent=True, stats=True, oc=3, out_ch=1):
    zs = [torch.from_numpy(np.array(z)).to(cuda) for z in members]
    out = torch.full((N, oh, ow, oc), FILL, dtype=torch.float32, device=cuda)
    p = torch.full((N, oh, ow, oc), FILL, dtype=torch.float32, device=cuda) if prob else None
    d = torch.full((N, oh, ow, oc), int(FILL), dtype=torch.uint8, device=cuda) if dissent else None
    s = torch.full((N, 4), -1, dtype=torch.int32, device=cuda) if stats else None      # the launch clears it on the stream
    r = None if rows is None else torch.from_numpy(rows).to(cuda)
    c = None if cols is None else torch.from_numpy(cols).to(cuda)
    vote.vote_logits(zs, channels, views, out, out_ch, r, c, MODE_NAMES[mode], prob=p, dissent=d, stats=s)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()                             # noqa: E731
    return host(out), host(p), host(d), host(s)


def _untouched(a, out_ch):
    return all((a[..., k] == FILL).all() for k in range(a.shape[-1]) if k != out_ch)


@pytest.mark.parametrize('case', VC.CASES, ids=VC.IDS)
def test_vote_assemble_equals_the_reference(cuda, case):
    members, classes, channels, rows, cols = VC.inputs(case)
    ref = VC.reference(case)
    M = len(case.views)
    out, prob, dissent, stats = _run(cuda, members, channels, case.views, case.N, case.oh, case.ow, case.mode, rows, cols)
    err = np.abs(prob[..., 1].astype(np.float64) - ref['pbar']).max()
    print(f'{case.id}: max |prob - pbar64| = {err:.3e} (bound {VC.prob_bound(M):.3e}), set {int(ref["mask"].sum())}, disputed {int(ref["stats"][:, 1].sum())}')
    assert np.array_equal(out[..., 1], ref['mask'].astype(np.float32))
    assert np.array_equal(dissent[..., 1].astype(np.int64), ref['dissent'])
    assert np.array_equal(stats.astype(np.int64), ref['stats'])
    assert err <= VC.prob_bound(M)
    assert _untouched(out, 1) and _untouched(prob, 1) and _untouched(dissent, 1)
    # each optional output null in turn: the others do not change
    for drop in ('prob', 'dissent', 'stats'):
        keep = {k: k != drop for k in ('prob', 'dissent', 'stats')}
        o2, p2, d2, s2 = _run(cuda, members, channels, case.views, case.N, case.oh, case.ow, case.mode, rows, cols, **keep)
        assert np.array_equal(o2, out)
        assert (p2 is None) if drop == 'prob' else np.array_equal(p2, prob)
        assert (d2 is None) if drop == 'dissent' else np.array_equal(d2, dissent)
        assert (s2 is None) if drop == 'stats' else np.array_equal(s2, stats)


@pytest.mark.parametrize('shape,osz', [((33, 33), (50, 41)), ((24, 40), (24, 40))])
def test_a_viewed_member_votes_like_the_frame_itself(cuda, shape, osz):
    """One member whose logits are view_v(Z), voted with code v, gives exactly the outputs of Z with code 0."""
    rng = np.random.default_rng(5)
    Z = VC.draw_logits(rng, (2, 2) + shape)
    base = _run(cuda, [Z], [1], [0], 2, osz[0], osz[1], 0)
    for v in range(8 if shape[0] == shape[1] else 4):
        got = _run(cuda, [R.view(Z, v)], [1], [v], 2, osz[0], osz[1], 0)
        for a, b in zip(got, base):
            assert np.array_equal(a, b), v


@pytest.mark.parametrize('tables', [False, True])
def test_one_member_equals_mask_assemble_bit_for_bit(cuda, tables):
    from oct_segmentation_amd.predict import cv2_nearest_index
    g = torch.Generator().manual_seed(3)
    z = (torch.randn((3, 2, 64, 64), generator=g) * 3).to(cuda)
    z[0, 1, :4] = torch.tensor([0.0, -0.0, 1e-9, -1e-9], device=cuda).repeat(16)          # the threshold itself: whatever the one sigmoid says
    oh, ow = 100, 75
    rows = torch.from_numpy(cv2_nearest_index(64, oh)).to(cuda) if tables else None
    cols = torch.from_numpy(cv2_nearest_index(64, ow)).to(cuda) if tables else None
    want = torch.zeros((3, oh, ow, 4), dtype=torch.float32, device=cuda)
    L.check(L.lib().octseg_mask_assemble(L.ptr(z), 3, 2, 64, 64, 1, L.ptr(want), oh, ow, 4, 2, L.ptr(rows), L.ptr(cols), L.stream_ptr()))
    for mode in MODE_NAMES:
        got = torch.zeros_like(want)
        dissent = torch.full((3, oh, ow, 4), 9, dtype=torch.uint8, device=cuda)
        vote.vote_logits([z], [1], [0], got, 2, rows, cols, mode, dissent=dissent)
        assert torch.equal(got, want) and got[..., 2].any() and not got[..., 2].all()
        assert not dissent[..., 2].any()


def test_view_batch_is_the_torch_expression(cuda):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 3, 8, 8), generator=g).to(cuda)
    for code in range(8):
        y = x
        if code & 4:
            y = y.transpose(-1, -2)
        if code & 2:
            y = y.flip(-2)
        if code & 1:
            y = y.flip(-1)
        got = vote.view_batch(x, code)
        assert got.is_contiguous() and torch.equal(got, y)
        assert np.array_equal(got.cpu().numpy(), R.view(x.cpu().numpy(), code))
    rect = torch.randn((1, 1, 4, 6), generator=g).to(cuda)
    assert torch.equal(vote.view_batch(rect, 3), rect.flip(-2).flip(-1))
    with pytest.raises(ValueError, match='square'):
        vote.view_batch(rect, 4)


# ------------------------------------------------------------------ end to end
SPECS = {'LM': ('unet', ['Lumen']), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap']), 'VV': ('unet', ['Vasa vasorum'])}
ALL = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']


def _checkpoint(cuda, d, key, seed):
    from oct_segmentation_amd.model import OCTSegmentationModel
    arch, classes = SPECS[key]
    os.makedirs(d)
    m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=seed, compute_dtype=torch.float32)
    m.save_checkpoint(os.path.join(d, 'weights.ckpt'))
    with open(os.path.join(d, 'config.json'), 'w') as f:
        json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': 64, 'classes': classes}, f)


def _frames():
    from PIL import Image
    rng = np.random.default_rng(0)
    return [Image.fromarray(rng.integers(0, 255, (80, 80, 3), dtype=np.uint8)) for _ in range(3)]


def _stats_from_maps(res, members):
    """The [n, 4, 4] counts taken from the returned maps with torch."""
    from oct_segmentation_amd.model import CLASS_IDS
    n = res.stack.shape[0]
    want = torch.zeros((n, 4, 4), dtype=torch.int64, device=res.stack.device)
    for name, M in members.items():
        c = CLASS_IDS[name] - 1
        mask, dis = res.stack[..., c] != 0, res.dissent[..., c].long()
        votes = torch.where(mask, M - dis, dis)
        disputed = (votes > 0) & (votes < M)
        want[:, c] = torch.stack([mask.sum((1, 2)), disputed.sum((1, 2)), (disputed & mask).sum((1, 2)), dis.sum((1, 2))], dim=1)
    return want


def test_voted_stack_without_folds_or_views_is_segment_stack(cuda, tmp_path):
    """(a) no fold directories, tta='none': the stack equals segment_stack's exactly; (b) fold_1 and fold_2 holding the same checkpoint: the same
    stack, no dissent, nothing disputed."""
    import shutil
    from oct_segmentation_amd.predict import segment_stack
    root = str(tmp_path / 'single')
    for i, key in enumerate(SPECS):
        _checkpoint(cuda, os.path.join(root, key), key, 20 + i)
    images = _frames()
    want = segment_stack(images, [96, 96], ALL, root, device='cuda', compute_dtype=torch.float32, device_preprocess=True, batch_size=2)
    res = vote.segment_stack_voted(images, [96, 96], ALL, root, tta='none', folds=True, device='cuda', compute_dtype=torch.float32, batch_size=2,
                                   want_dissent=True, want_prob=True)
    assert res.members == {k: 1 for k in ALL} and res.stats.shape == (3, 4, 4) and res.stats.dtype == torch.int32
    assert torch.equal(res.stack, want) and want.any()
    assert not res.dissent.any() and not res.stats[:, :, 1:].any()
    assert torch.equal(res.stats[:, :, 0].long(), want.sum((1, 2)).long())
    assert torch.equal(res.prob > 0.5, want != 0)
    twin = str(tmp_path / 'twin')
    for key in SPECS:
        for k in (1, 2):
            shutil.copytree(os.path.join(root, key), os.path.join(twin, key, f'fold_{k}'))
    res2 = vote.segment_stack_voted(images, [96, 96], ALL, twin, tta='none', folds=True, device='cuda', compute_dtype=torch.float32, batch_size=2,
                                    want_dissent=True)
    assert res2.members == {k: 2 for k in ALL} and res2.prob is None
    assert torch.equal(res2.stack, want) and not res2.dissent.any() and not res2.stats[:, :, 1:].any()
    assert torch.equal(res2.stats[:, :, 0].long(), want.sum((1, 2)).long())


@pytest.fixture(scope='module')
def two_folds(cuda, tmp_path_factory):
    root = str(tmp_path_factory.mktemp('folds'))
    for i, key in enumerate(SPECS):
        for k in (1, 2):
            _checkpoint(cuda, os.path.join(root, key, f'fold_{k}'), key, 30 + 10 * k + i)
    return root


@pytest.mark.parametrize('mode', MODE_NAMES)
def test_voted_stack_equals_vote_logits_on_logits_gathered_by_hand(cuda, two_folds, mode):
    """(c) two seeds as folds and tta='flips': M = 8 per class.  GPU against GPU: the eager forward is bit-reproducible."""
    from oct_segmentation_amd.model import CLASS_IDS
    from oct_segmentation_amd.predict import MODELS_META, _resize_frames_on_device, _upload_frames_u8, cv2_nearest_index, load_model
    images = _frames()
    asked = ['Lumen', 'Fibrous cap', 'Lipid core']
    res = vote.segment_stack_voted(images, [96, 96], asked, two_folds, tta='flips', folds=True, mode=mode, device='cuda',
                                   compute_dtype=torch.float32, want_dissent=True, want_prob=True)      # (one batch, as gathered below)
    assert res.members == {k: 8 for k in asked}
    frames = _upload_frames_u8(images, 'cuda')
    x = _resize_frames_on_device(frames, 0, 3, 64)
    rows = torch.from_numpy(cv2_nearest_index(64, 96)).to(cuda)
    stack = torch.zeros((3, 96, 96, 4), dtype=torch.float32, device=cuda)
    dissent = torch.zeros((3, 96, 96, 4), dtype=torch.uint8, device=cuda)
    prob = torch.zeros_like(stack)
    stats = torch.zeros((3, 4, 4), dtype=torch.int32, device=cuda)
    for key in ('LM', 'FC_LC'):
        nets = [load_model(os.path.join(two_folds, key, f'fold_{k}'), 'cuda', torch.float32)[0] for k in (1, 2)]
        logits = [net.predict_logits(vote.view_batch(x, v)) for net in nets for v in (0, 1, 2, 3)]
        for name in asked:
            if MODELS_META[name]['model_dir'] != key:
                continue
            c = CLASS_IDS[name] - 1
            s = torch.zeros((3, 4), dtype=torch.int32, device=cuda)
            vote.vote_logits(logits, [MODELS_META[name]['index']] * 8, [0, 1, 2, 3] * 2, stack, c, rows, rows, mode, prob=prob, dissent=dissent, stats=s)
            stats[:, c] = s
    assert torch.equal(res.stack, stack) and torch.equal(res.dissent, dissent) and torch.equal(res.stats, stats) and torch.equal(res.prob, prob)
    assert torch.equal(res.stats.long(), _stats_from_maps(res, res.members))
    assert res.stats[:, :3, 1].sum() > 0 and res.dissent.any()                            # different seeds do disagree
    assert not res.stack[..., 3].any() and not res.dissent[..., 3].any() and not res.stats[:, 3].any()      # Vasa vasorum was not asked for
    assert int(res.dissent.max()) <= (4 if mode == 'majority' else 7)


def test_predict_main_writes_the_vote_files(cuda, two_folds, tmp_path):
    """(d) predict.main with folds=true tta=flips dissent_maps=true: vote.json (its numbers are the stats), the dissent PNGs and the usual two PNGs
    per frame; with no extra key, no vote.json."""
    from PIL import Image
    from oct_segmentation_amd import predict
    from oct_segmentation_amd.model import CLASS_IDS
    data = tmp_path / 'in'
    data.mkdir()
    names = ['c_3', 'a_1', 'b_2']
    for name, img in zip(names, _frames()):
        img.save(str(data / f'{name}.png'))
    classes = ['Lumen', 'Lipid core', 'Fibrous cap']
    common = [f'data_dir={data}', 'output_size=[96,96]', 'compute_dtype=fp32', f'classes={json.dumps(classes)}']
    single = tmp_path / 'single_models'
    for key in ('LM', 'FC_LC'):
        os.makedirs(single / key)
        for f in ('config.json', 'weights.ckpt'):
            os.link(os.path.join(two_folds, key, 'fold_1', f), single / key / f)
    plain = tmp_path / 'plain'
    assert predict.main(common + [f'models_dir={single}', f'save_dir={plain}']) == 0
    assert sorted(os.listdir(plain)) == sorted(f'{n}_{k}.png' for n in names for k in ('mask', 'overlay'))      # no vote.json
    with pytest.raises(ValueError, match='dissent_maps'):                                 # a dissent map of one member would be a blank promise
        predict.main(common + [f'models_dir={single}', f'save_dir={plain}', 'dissent_maps=true'])

    out = tmp_path / 'voted'
    assert predict.main(common + [f'models_dir={two_folds}', f'save_dir={out}', 'folds=true', 'tta=flips', 'dissent_maps=true']) == 0
    assert sorted(os.listdir(out)) == sorted([f'{n}_{k}.png' for n in names for k in ('mask', 'overlay', 'dissent')] + ['vote.json'])
    report = json.load(open(out / 'vote.json'))
    paths = predict._image_paths(str(data))
    images = predict._frames_on_device(paths, [96, 96], 'cuda')
    res = vote.segment_stack_voted(images, [96, 96], classes, two_folds, tta='flips', folds=True, device='cuda', compute_dtype=torch.float32,
                                   want_dissent=True)
    stats = res.stats.cpu().numpy()
    by_name = {os.path.basename(p).split('.')[0]: i for i, p in enumerate(paths)}
    for cls in classes:
        entry = report['classes'][cls]
        assert entry['members'] == 8 and list(entry['slices']) == sorted(names)
        for name, row in entry['slices'].items():
            want = stats[by_name[name], CLASS_IDS[cls] - 1]
            assert [row[k] for k in vote.STAT_COLUMNS] == want.tolist()
            assert row['disputed_ratio'] == want[1] / max(want[0], 1)
    maps = vote.dissent_images(res, classes)
    for name in names:
        png = np.asarray(Image.open(out / f'{name}_dissent.png'))
        assert png.dtype == np.uint8 and png.shape == (96, 96) and np.array_equal(png, maps[by_name[name]])
    want = (res.dissent[..., :3].long() * (255 // 8)).amax(dim=-1).cpu().numpy()
    assert np.array_equal(maps, want) and maps.any()
