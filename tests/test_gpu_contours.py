"""Mask outlines on the GPU (csrc/contours.hip through oct_segmentation_amd/contours.py) against the sequential crack follower of
tests/contours_ref.py, which tests/test_contours.py proves against scipy.ndimage and matplotlib.path on these very cases.  Every comparison is
integer equality: there is no tolerance in this feature."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from matplotlib.path import Path
from PIL import Image

import contours_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import cleanup, contours, shape
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 129), (130, 97), (300, 257)]


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded(h, w):
    """The issue's stacks: [3, h, w, 4] at densities 0.5, 0.01, empty, full; at (300, 257) only the 0.01 and the full channel.  Read-only."""
    st = R.seeded_stack(h, w, channels=(0.01, 1.0) if (h, w) == (300, 257) else (0.5, 0.01, 0.0, 1.0))
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def ref(h, w):
    return R.trace_stack(seeded(h, w))


def plane_stack(m):
    return np.asarray(m, np.float32)[None, :, :, None]


def same(cont, want):
    ncont, table, verts = want[:3]
    assert cont.ncont.dtype == cont.table.dtype == cont.vertices.dtype == torch.int32
    assert np.array_equal(host(cont.ncont), ncont)
    got_t, got_v = host(cont.table), host(cont.vertices)
    assert got_t.shape == table.shape and got_v.shape == verts.shape
    for k, name in enumerate(R.FIELDS):
        assert np.array_equal(got_t[:, k], table[:, k]), name
    assert np.array_equal(got_v, verts)


# ---- 1. seeded stacks
@pytest.mark.parametrize('h,w', SHAPES)
def test_seeded_stacks_equal_the_reference(h, w):
    st = seeded(h, w)
    d = dev(st)
    counts = contours.count_stack(d)
    assert counts.dtype == torch.int64 and np.array_equal(host(counts), ref(h, w)[3])
    assert np.array_equal(host(counts[..., 0]), host(shape.moments_stack(d)[..., 10]))                # EDGES
    cont = contours.trace_stack(d)
    same(cont, ref(h, w))
    assert cont.size == (w, h)


# ---- 2. patterns
@functools.lru_cache(maxsize=None)
def pattern_cases():
    return R.patterns()


@pytest.mark.parametrize('name', sorted(R.patterns()))
def test_patterns(name):
    m = pattern_cases()[name]
    st = plane_stack(m)
    want = R.trace_stack(st)
    if name == 'checkerboard':
        assert want[0][0, 0] == 32 and want[2].shape[0] == 200
    if name in ('staircase', 'spiral') or name.startswith(('bar', 'column')):
        assert want[0][0, 0] == 1
    if name == 'rings':
        assert want[0][0, 0] == 3
    if name.startswith(('bar', 'column')):
        assert want[1][0, 4] == 2 * int(''.join(ch for ch in name if ch.isdigit())) + 2      # 2 L + 2 straddles the powers of two
    d = dev(st)
    assert np.array_equal(host(contours.count_stack(d)), want[3])
    same(contours.trace_stack(d), want)


# ---- 3. cross-checks within the product
@pytest.mark.parametrize('h,w', [(37, 53), (65, 129), (130, 97)])
def test_labels_and_areas_agree_with_the_clean_up(h, w):
    st = seeded(h, w)
    d = dev(st)
    cont = contours.trace_stack(d)
    labels = host(cleanup.label_stack(d, connectivity=8))                                              # [N, C, H, W]
    table, verts = host(cont.table), host(cont.vertices)
    n, sc = labels.shape[:2]
    for row in table:
        x, y = verts[row[1]]
        px = x if row[3] > 0 else x - 1                        # an outer leader runs east over its pixel, a hole's runs south beside its pixel
        assert labels[row[0] // sc, row[0] % sc, y, px] == row[9]
    ncomp, top = (host(t) for t in cleanup.component_table(d))
    polys = cont.polygons()
    shapes = contours.component_shapes(cont)
    for i in range(n):
        for c in range(sc):
            assert len(polys[i][c]) == ncomp[i, c]
            area = {p['label']: p['area'] for p in polys[i][c]}
            for k in range(min(int(ncomp[i, c]), 8)):          # the 8 that component_table ranks
                assert area[1 + int(top[i, c, k, 1])] == int(top[i, c, k, 0])
                assert shapes[i][c][k]['label'] == 1 + int(top[i, c, k, 1]) and shapes[i][c][k]['area'] == int(top[i, c, k, 0])


# ---- 4. plumbing
def test_chunks_give_the_same_contours_and_two_runs_are_bit_equal():
    h, w = 65, 129
    d = dev(seeded(h, w))
    one = contours.trace_stack(d)
    again = contours.trace_stack(d)
    for a, b in zip(one[:3], again[:3]):
        assert torch.equal(a, b)
    edges = host(contours.count_stack(d)).sum(axis=1)[:, 0]
    per_slice = max(int(L.lib().octseg_contours_scratch_bytes(4, h, w, int(e))) for e in edges)
    assert contours._slices_per_chunk([int(e) for e in edges], h, w, 4, per_slice) == 1                 # three chunks
    for budget in (per_slice, 1):                                                                      # (1: not even one slice fits -> slice by slice)
        got = contours.trace_stack(d, scratch_bytes=budget)
        for a, b in zip(one[:3], got[:3]):
            assert torch.equal(a, b), budget
    same(one, ref(h, w))
    # a stack with an empty slice in the middle: the chunk's placeholder row must not shift the later chunks
    st = np.array(seeded(37, 53))
    st[1] = 0
    same(contours.trace_stack(dev(st), scratch_bytes=1), R.trace_stack(st))


def test_overflow_stores_nothing_past_a_buffer_and_refused_calls_launch_nothing():
    h, w = 37, 53
    st = seeded(h, w)
    d = dev(st)
    before = d.clone()
    ncont, table, verts, counts = ref(h, w)
    e, c, v = int(counts[..., 0].sum()), int(table.shape[0]), int(verts.shape[0])
    lib = L.lib()
    s = L.stream_ptr()

    def run(ecap, ccap, vcap, scratch_fill=0x55):
        need = int(lib.octseg_contours_scratch_bytes(12, h, w, ecap))
        scratch = torch.full((need + 4096,), scratch_fill, dtype=torch.uint8, device='cuda')           # + a guard inside the same allocation
        nc = torch.full((13,), 7, dtype=torch.int32, device='cuda')
        tb = torch.full((ccap + 16, contours.NFIELDS), 7, dtype=torch.int32, device='cuda')
        vs = torch.full((vcap + 16, 2), 7, dtype=torch.int32, device='cuda')
        ov = torch.zeros((2,), dtype=torch.int32, device='cuda')
        ov[1] = 7
        L.check(lib.octseg_stack_contours(L.ptr(d), 3, h, w, 4, L.ptr(scratch), need, ecap, ccap, vcap, L.ptr(nc), L.ptr(tb), L.ptr(vs), L.ptr(ov), s))
        torch.cuda.synchronize()
        assert (scratch[need:] == scratch_fill).all() and int(nc[12]) == 7 and (tb[ccap:] == 7).all() and (vs[vcap:] == 7).all() and int(ov[1]) == 7
        return host(nc[:12]).reshape(3, 4), host(tb[:ccap]), host(vs[:vcap]), int(ov[0])

    for fill in (0x00, 0xFF, 0x55):                            # exact capacities; the scratch is work space only
        nc, tb, vs, ov = run(e, c, v, fill)
        assert ov == 0 and np.array_equal(nc, ncont) and np.array_equal(tb, table) and np.array_equal(vs, verts)
    nc, tb, vs, ov = run(e + 100, c + 3, v + 5)                 # rows beyond the total are left alone
    assert ov == 0 and np.array_equal(tb[:c], table) and (tb[c:] == 7).all() and np.array_equal(vs[:v], verts) and (vs[v:] == 7).all()
    nc, tb, vs, ov = run(e - 1, c, v)                           # one edge short: nothing is traced
    assert ov == 1 and (nc == 0).all() and (tb == 7).all() and (vs == 7).all()
    nc, tb, vs, ov = run(e, c - 1, v)                           # one contour short: the rows that fit are complete
    assert ov == 1 and np.array_equal(nc, ncont) and np.array_equal(tb, table[:c - 1]) and np.array_equal(vs, verts)
    nc, tb, vs, ov = run(e, c, v - 1)                           # one vertex short
    assert ov == 1 and np.array_equal(nc, ncont) and np.array_equal(tb, table) and np.array_equal(vs, verts[:v - 1])
    # refusals: nothing may be written
    need = int(lib.octseg_contours_scratch_bytes(12, h, w, e))
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    nc = torch.full((12,), 7, dtype=torch.int32, device='cuda')
    tb = torch.full((c, contours.NFIELDS), 7, dtype=torch.int32, device='cuda')
    vs = torch.full((v, 2), 7, dtype=torch.int32, device='cuda')
    ov = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    cn = torch.full((12, 2), 7, dtype=torch.int64, device='cuda')
    P = L.ptr
    assert lib.octseg_stack_contours(P(d), 3, h, w, 4, P(scratch), need - 1, e, c, v, P(nc), P(tb), P(vs), P(ov), s) == -5
    assert lib.octseg_stack_contours(P(d), 3, h, w, 4, None, need, e, c, v, P(nc), P(tb), P(vs), P(ov), s) == -5
    assert lib.octseg_stack_contours(P(d), 3, h, w, 4, P(scratch), need, e, 0, v, P(nc), P(tb), P(vs), P(ov), s) == -5
    assert lib.octseg_stack_contours(P(d), 3, h, w, 4, P(scratch), need, e, c, 2 ** 31, P(nc), P(tb), P(vs), P(ov), s) == -5
    assert lib.octseg_stack_contours(P(d), 3, 0, w, 4, P(scratch), need, e, c, v, P(nc), P(tb), P(vs), P(ov), s) == -1
    assert lib.octseg_stack_contours(P(d), 3, h, w, 17, P(scratch), need, e, c, v, P(nc), P(tb), P(vs), P(ov), s) == -1
    assert lib.octseg_stack_contour_counts(P(d), 3, h, w, 4, None, s) == -5
    assert lib.octseg_stack_contour_counts(P(d), 3, h, 0, 4, P(cn), s) == -1
    torch.cuda.synchronize()
    assert (nc == 7).all() and (tb == 7).all() and (vs == 7).all() and (ov == 7).all() and (cn == 7).all()
    assert torch.equal(d, before)                               # the input stack is never modified


def test_non_contiguous_and_misaligned_stacks():
    h, w = 37, 53
    st = seeded(h, w)
    want = ref(h, w)
    wide = torch.zeros((3, h, w, 6), device='cuda')
    wide[..., 1:5] = dev(st)
    view = wide[..., 1:5]                                       # not contiguous: copied, as cleanup._check does
    assert not view.is_contiguous()
    same(contours.trace_stack(view), want)
    assert np.array_equal(host(contours.count_stack(view)), want[3])
    flat = torch.zeros((st.size + 1,), device='cuda')
    flat[1:] = dev(st).reshape(-1)
    off = flat[1:].view(3, h, w, 4)                             # contiguous but 4 bytes off a 16-byte boundary: the scalar loads
    assert off.data_ptr() % 16 == 4
    same(contours.trace_stack(off), want)
    assert np.array_equal(host(contours.count_stack(off)), want[3])
    three = np.ascontiguousarray(st[..., :3])                   # three channels: the scalar path on an aligned base
    same(contours.trace_stack(dev(three)), R.trace_stack(three))
    for bad in (torch.zeros((2, 4, 4, 4), dtype=torch.float64, device='cuda'), torch.zeros((4, 4, 4), device='cuda'),
                torch.zeros((2, 0, 4, 4), device='cuda'), torch.zeros((2, 4, 4, 17), device='cuda')):
        for fn in (contours.count_stack, contours.trace_stack, contours.component_shapes, contours.contour_report):
            with pytest.raises(ValueError):
                fn(bad)


# ---- 5. the served products
def fill(polys, h, w):
    """The even-odd fill of a plane's polygons at the pixel centres."""
    yy, xx = np.mgrid[0:h, 0:w]
    pts = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], axis=1)
    out = np.zeros(h * w, bool)
    for p in polys:
        for ring in [p['exterior']] + p['interior']:
            out ^= Path(np.asarray(ring, float)).contains_points(pts)
    return out.reshape(h, w)


def test_analyze_stack_with_contours():
    from oct_segmentation_amd import analysis
    st = np.zeros((3, 40, 48, 4), np.float32)
    st[0, 5:20, 6:30, 0] = 1
    st[0, 9:12, 10:14, 0] = 0
    st[2, 1:4, 1:4, 0] = 1
    st[1, 10:30, 10:30, 1] = 1
    d = dev(st)
    plain = analysis.analyze_stack(d)
    got = analysis.analyze_stack(d, with_contours=True)
    assert got.pop('contour_convention') == contours.CONVENTION
    for name, cid in CLASS_IDS.items():
        lists = got['objects'][name].pop('contours')
        assert len(lists) == len(got['objects'][name]['slice'])
        for idx, polys in zip(got['objects'][name]['slice'], lists):
            assert np.array_equal(fill(polys, 40, 48), st[idx, :, :, cid - 1] != 0)
    assert got == plain
    json.dumps(analysis.analyze_stack(d, with_contours=True))
    with pytest.raises(NotImplementedError):
        analysis.analyze_stack(d, thickness='contour', with_contours=True)


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


def test_predict_main_writes_contours_json(cuda, tmp_path):
    """Two synthetic frames through the command line, image files and a .npy volume: the polygons fill back to the served masks."""
    from oct_segmentation_amd import predict, pullback
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(29)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first']                              # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'clean=true']
    off, on = os.path.join(tmp_path, 'off'), os.path.join(tmp_path, 'on')
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={on}', 'contours=true']) == 0
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ['contours.json'])
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = cleanup.clean_stack(predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32,
                                                      device_preprocess=True))
    with open(os.path.join(on, 'contours.json')) as f:
        got = json.load(f)
    assert got == json.loads(json.dumps(contours.contour_report(stack, names)))
    assert got['convention'] == contours.CONVENTION and (got['width'], got['height']) == (120, 120) and [s['name'] for s in got['slices']] == names
    served = host(stack) != 0
    assert served.any()
    for i, sl in enumerate(got['slices']):
        for c, cls in enumerate(got['classes']):
            assert np.array_equal(fill(sl['objects'][cls], 120, 120), served[i, :, :, c])
    # the volume path
    vol = rng.integers(0, 256, (2, 90, 90, 3), dtype=np.uint8)
    np.save(os.path.join(tmp_path, 'pull.npy'), vol)
    von = os.path.join(tmp_path, 'von')
    assert predict.main([f'data_dir={os.path.join(tmp_path, "pull.npy")}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32',
                         f'save_dir={von}', 'contours=true']) == 0
    res = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32)
    with open(os.path.join(von, 'contours.json')) as f:
        assert json.load(f) == json.loads(json.dumps(contours.contour_report(res.stack, ['pull_001', 'pull_002'])))
