"""Centreline pruning without a GPU: the numpy restatement (tests/prune_ref.py) against scipy.ndimage's conditional dilation, propagation and
component and hole counts, the hand cases and the demo excerpt; the ABI signatures and refusals, the host half of
oct_segmentation_amd/skeleton.py and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import distance_ref
import prune_cases as Q
import prune_ref as P
import skeleton_cases as K
import skeleton_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import skeleton

ONES = np.ones((3, 3), bool)


def components(m):
    return ndimage.label(m, structure=np.ones((3, 3), int))[1]


def holes(m):
    """4-connected components of the complement of the plane padded by one clear ring, minus the outside."""
    return ndimage.label(~np.pad(m, 1, constant_values=False))[1] - 1


def has_block(m):
    return bool((m[:-1, :-1] & m[:-1, 1:] & m[1:, :-1] & m[1:, 1:]).any())


# ---- 1. the restatement against scipy.ndimage, and what a pruning must keep
SKELETONS = list(Q.skeletons())


def pruned(a, spur, trim):
    """``(out, census)`` of one plane by the restatement, cached by content (tests/prune_cases.py)."""
    out, cen = Q.reference(a[None, :, :, None], spur, trim)
    return out[0, :, :, 0] != 0, cen[0, 0]


@pytest.mark.parametrize('name,a,kind', SKELETONS, ids=[s[0] for s in SKELETONS])
def test_restatement_against_ndimage(name, a, kind):
    assert np.array_equal(P.prune(a, 0, 0)[0], a) and not P.prune(a, 0, 0)[1].any()          # (0, 0) is the identity
    for spur, trim in Q.PAIRS:
        x, y, z, r = P.stages(a, spur, trim)
        if spur > 0:
            t = P.tips(x)
            want = ndimage.binary_dilation(t, ONES, iterations=spur, mask=a) if t.any() else t
            assert np.array_equal(P.grow(t, spur, a), want), (name, spur)
            assert np.array_equal(y, x | want)
        else:
            assert np.array_equal(y, a)
        assert np.array_equal(r, ndimage.binary_propagation(z, ONES, mask=a)), (name, spur, trim)
        out, cen = pruned(a, spur, trim)
        rest = a & ~r
        assert np.array_equal(out, z | rest) and np.array_equal(P.prune(a, spur, trim)[1], rest)
        assert not (out & ~a).any()                                                          # a subset of the input
        assert components(out) == components(a), (name, spur, trim)
        assert holes(out) == holes(a), (name, spur, trim)
        assert cen[0] == a.sum() and cen[1] == out.sum() and cen[8] == rest.sum()
        k = ndimage.convolve(out.astype(np.int32), np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]]), mode='constant')
        assert cen[3:6].tolist() == [int((out & (k == 1)).sum()), int((out & (k >= 3)).sum()), int((out & (k == 0)).sum())]


def test_euler_relation_on_outputs_without_a_block():
    """On a plane without a 2 x 2 block of set pixels, pixels - orth - diag = components - holes.  At least 40 outputs must qualify."""
    count = {'blobs': 0, 'drawn': 0}
    for name, a, kind in SKELETONS:
        for spur, trim in Q.PAIRS:
            out, cen = pruned(a, spur, trim)
            if out.any() and not has_block(out):
                assert cen[1] - cen[6] - cen[7] == components(out) - holes(out), (name, spur, trim)
                count[kind] += 1
    assert count['blobs'] + count['drawn'] >= 40, count


def test_one_pass_never_cuts_or_loses_more_than_a_two_pixel_component():
    """One erosion pass keeps the holes, and changes the component count only by removing whole two-pixel components (two tips facing each
    other): the one case the restore rule exists for."""
    for name, a, _ in SKELETONS:
        b = P.erode(a, 1)
        lab, n = ndimage.label(a, structure=np.ones((3, 3), int))
        sizes = ndimage.sum(a, lab, np.arange(1, n + 1)) if n else np.zeros(0)
        lost = [c for c in range(1, n + 1) if not b[lab == c].any()]
        assert all(sizes[c - 1] == 2 for c in lost), name
        assert components(b) == n - len(lost) and holes(b) == holes(a), name


# ---- 2. hand cases: the values of the run made while the feature was specified
def test_hand_cases():
    for name, m, spur, trim, pixels, tips, links, restored in Q.hand_values():
        cen = P.census(m, spur, trim)
        assert cen[0] == m.sum() and cen[1] == pixels and (cen[6], cen[7]) == links and cen[8] == restored, (name, spur, trim, cen.tolist())
        if tips is not None:
            assert cen[2] == tips, (name, spur, trim)
    stub = Q.stub()
    assert np.array_equal(P.prune(stub, 2, 0)[0], stub)                                      # a 3-pixel stub survives spur = 2
    cut = P.prune(stub, 3, 0)[0]
    assert not cut[1:4, 10].any() and cut[4, 2:22].all()                                     # and goes at 3, the row at full length
    assert np.array_equal(np.nonzero(P.prune(stub, 3, 2)[0][4])[0], np.arange(4, 20))
    assert np.array_equal(P.prune(stub, 0, 12)[1], stub)
    one = np.zeros((5, 5), bool)
    one[2, 2] = True
    assert not P.tips(one).any() and np.array_equal(P.prune(one, 5, 5)[0], one)              # an isolated pixel is not a tip
    row = np.zeros((5, 9), bool)
    row[3, 1:8] = True
    row[2, 4] = True                                                                         # a one-pixel stub on a row: a tip with three neighbours
    assert P.tips(row)[2, 4] and P.neighbour_count(row)[2, 4] == 3 and not P.prune(row, 1, 0)[0][2, 4]
    ring = Q.thin_ring()
    assert not P.tips(ring).any() and np.array_equal(P.prune(ring, 10, 10)[0], ring) and P.census(ring, 10, 10)[8] == 0
    assert P.census(np.zeros((5, 9), bool), 3, 3).tolist() == [0] * 9
    assert P.length(np.array([0, 0, 0, 0, 0, 0, 3, 2, 0])) == 3 + 2 * np.sqrt(2.0)


# ---- 3. the demo excerpt's cap planes
def test_demo_excerpt_values():
    skel = Q.excerpt_skeleton()
    stack = K.excerpt_stack()
    caps = [skel[i, :, :, K.CAP] != 0 for i in range(3)]
    cen0 = [P.census(c, 0, 0) for c in caps]
    assert [int(c[1]) for c in cen0] == [444, 542, 378]
    assert [(int(c[6]), int(c[7])) for c in cen0] == [(286, 157), (319, 222), (233, 144)]
    cut = [P.prune(c, 0, 20)[0] for c in caps]
    assert [int(c.sum()) for c in cut] == [358, 464, 318]
    mins = []
    for i in range(3):
        full = distance_ref.edt2(~stack[i, :, :, K.CAP])
        assert 2 * np.sqrt(full[caps[i]].min()) - 1 == pytest.approx(7.2462, abs=1e-4)      # the taper's last pixel: 2 sqrt(17) - 1
        mins.append(2 * np.sqrt(full[cut[i]].min()) - 1)
    assert mins == pytest.approx([19.59, 19.59, 21.80], abs=5e-3)
    c10 = P.census(caps[0], 10, 0)
    assert c10[1] == 435 and c10[2] == 4
    for c, o in zip(caps, cut):
        assert components(o) == components(c) and holes(o) == holes(c)


# ---- 4. ABI
def test_symbols_of_the_prune_entry_points():
    i, p, z = C.c_int, C.c_void_p, C.c_size_t
    want = {'octseg_prune_scratch_bytes': (z, [i] * 4),
            'octseg_stack_prune': (i, [p, i, i, i, i, i, i, i, p, z, p, p, p])}
    for name, sig in want.items():
        assert L.SYMBOLS[name] == sig, name
        assert hasattr(L.lib(), name)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'octseg.h')).read()
    assert '#define OCTSEG_PRUNE_GLOBAL 1' in header and skeleton.PATHS == {'auto': 0, 'global': 1}
    assert 'size_t octseg_prune_scratch_bytes(int N, int H, int W, int channels);' in header
    assert 'int octseg_stack_prune(const float* skel, int N, int H, int W, int channels, int spur, int trim, int flags, void* scratch, ' \
           'size_t scratch_bytes,' in header
    for phrase in ('P2 & ~(P4|P5|P6|P7|P8)', 'no orthogonal neighbour is set and exactly one diagonal neighbour is set', 'X = erode(A, spur)',
                   'Y = X | grow(tips(X), spur, A)', 'Z = erode(Y, trim)', 'out = Z | (A & ~R)', 'w & SE & ~E & ~S', 'orth + sqrt(2) * diag'):
        assert phrase in header, phrase
    assert skeleton.PRUNE_COLUMNS == P.COLUMNS and len(skeleton.PRUNE_COLUMNS) == 9


def test_library_refuses_before_any_launch():
    lib = L.lib()
    fn, size = lib.octseg_stack_prune, lib.octseg_prune_scratch_bytes
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17), (-1, 8, 8, 1),
                (1 << 27, 8, 8, 2)):                                  # the last: N * channels * 9 reaches 2^31
        assert size(*bad) == 0, bad
    # four sets of bit planes at least: input, result, the parked plane, and the second image of the global path
    for n, h, w, c in ((2, 33, 65, 4), (1, 750, 750, 4), (1, 4096, 4096, 16), (3, 1, 1, 1)):
        assert size(n, h, w, c) >= 4 * n * c * h * ((w + 63) // 64) * 8
        assert size(n, h, w, c) <= 4 * (n * c * h * ((w + 63) // 64) * 8 + 256)                # and no more than that with the carver's alignment
    assert size(4, 33, 65, 4) >= 2 * size(2, 33, 65, 4) - 4 * 256                              # linear in the slices up to the alignment
    buf = (C.c_char * 4096)()                                # a host buffer: the calls below must return before they touch a pointer
    a = C.cast(buf, C.c_void_p)
    b = C.c_void_p(a.value + 256)
    odd = C.c_void_p(a.value + 4)
    big = 1 << 40
    BAD_SHAPE, BAD_ARG = -1, -5
    assert fn(None, 1, 8, 8, 1, 1, 1, 0, a, big, b, b, None) == BAD_ARG
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, None, big, b, b, None) == BAD_ARG
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, a, big, None, None, None) == BAD_ARG
    assert b'both null' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, b, big, a, None, None) == BAD_ARG        # out aliases the input
    assert b'alias' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, odd, big, b, None, None) == BAD_ARG
    assert b'aligned' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, a, 16, b, None, None) == BAD_ARG
    assert b'scratch is smaller' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 1, 1, 0, a, size(1, 8, 8, 1) - 1, b, None, None) == BAD_ARG
    for flags in (2, 3, 4, -1, 1 << 30):
        assert fn(a, 1, 8, 8, 1, 1, 1, flags, a, big, b, None, None) == BAD_ARG
        assert b'flag' in lib.octseg_last_error()
    for spur, trim in ((-1, 0), (0, -1), (8193, 0), (0, 8193), (1 << 30, 1), (-(1 << 31), 0)):
        assert fn(a, 1, 8, 8, 1, spur, trim, 0, a, big, b, None, None) == BAD_ARG, (spur, trim)
        assert b'0..8192' in lib.octseg_last_error()
    for n, h, w, c in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17), (1 << 27, 8, 8, 2)):
        assert fn(a, n, h, w, c, 1, 1, 0, a, big, b, None, None) == BAD_SHAPE, (n, h, w, c)
    assert not any(buf.raw)


# ---- 5. the wrappers' refusals and the host half
def test_wrappers_refuse_host_tensors_unknown_paths_and_bad_steps():
    cpu = torch.zeros((1, 4, 4, 4))
    for bad in (cpu, cpu.numpy(), cpu.double(), cpu[0]):
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            skeleton.prune_stack(bad, 1, 1)
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            skeleton.thickness_report(bad, spur=1)
    with pytest.raises(ValueError, match='path'):
        skeleton.prune_stack(cpu, path='lds')
    for kw in ({'spur': -1}, {'trim': 8193}, {'spur': 1.5}, {'trim': True}):
        with pytest.raises(ValueError, match='0..8192'):
            skeleton.prune_stack(cpu, **kw)
        with pytest.raises(ValueError, match='0..8192'):
            skeleton.thickness_report(cpu, **kw)
    cen = np.zeros((2, 3, 9), np.int32)
    cen[1, 2, 6:8] = (5, 2)
    length = skeleton.centreline_length(torch.from_numpy(cen))
    assert length.dtype == np.float64 and length.shape == (2, 3) and length[1, 2] == 5 + 2 * np.sqrt(2.0) and length.sum() == length[1, 2]
    assert np.array_equal(skeleton.centreline_length(cen), length)
    with pytest.raises(ValueError):
        skeleton.centreline_length(np.zeros((2, 3, 6), np.int32))


def test_build_pruned_thickness_on_hand_written_lists():
    # slice 0: class a = a 16-pixel row (d2 = 9 -> width 5) trimmed to 12, class b absent.
    # slice 1: class a fills its frame (one skeleton pixel, restored: DIST_NONE), class b = 4 pixels kept of 7, one diagonal link.
    none = skeleton.DIST_NONE
    d2 = [9] * 12 + [] + [none] + [1, 4, 4, 4]
    offsets = [0, 12, 12, 13, 17]
    census = [[[100, 16, 2, 0, 0, 2], [0, 0, 0, 0, 0, 0]], [[81, 1, 0, 0, 1, 4], [20, 7, 3, 1, 0, 1]]]
    pruned = [[[16, 12, 2, 2, 0, 0, 11, 0, 0], [0] * 9], [[1, 1, 0, 0, 0, 1, 0, 0, 1], [7, 4, 2, 2, 0, 0, 2, 1, 0]]]
    rep = skeleton.build_pruned_thickness(d2, offsets, census, pruned, ['a', 'b'])
    assert rep['a'] == {'slice': [0, 1], 'centreline': [12, 1], 'ends': [2, 0], 'junctions': [0, 0], 'passes': [2, 4],
                        'median': [5.0, None], 'mean': [5.0, None], 'min': [5.0, None], 'p5': [5.0, None], 'max': [5.0, None],
                        'tips': [2, 0], 'length': [11.0, 0.0], 'removed': [4, 0], 'restored': [0, 1]}
    b = rep['b']
    assert b['slice'] == [1] and b['centreline'] == [4] and b['ends'] == [2] and b['junctions'] == [0] and b['passes'] == [1]
    assert b['median'] == [3.0] and b['min'] == [1.0] and b['tips'] == [2] and b['removed'] == [3] and b['restored'] == [0]
    assert b['length'] == [2 + np.sqrt(2.0)]
    assert list(rep['a'])[:10] == list(skeleton.build_thickness([9] * 16 + [none] + [1] * 7, [0, 16, 16, 17, 24], census, ['a', 'b'])['a'])
    json.dumps(rep)
    half = skeleton.build_pruned_thickness(d2, offsets, census, pruned, ['a', 'b'], names=['s0', 's1'], ratio=2)
    assert half['a']['image'] == ['s0', 's1'] and half['a']['length'] == [5.5, 0.0] and half['b']['length'] == [(2 + np.sqrt(2.0)) / 2]
    assert half['a']['median'] == [2.5, None] and half['a']['centreline'] == [12, 1] and half['a']['removed'] == [4, 0]
    with pytest.raises(ValueError):
        skeleton.build_pruned_thickness(d2, offsets, census, pruned, ['a', 'b'], ratio=0)
    with pytest.raises(ValueError):
        skeleton.build_pruned_thickness(d2, offsets, census, [p[:1] for p in pruned], ['a', 'b'])
    with pytest.raises(ValueError):
        skeleton.build_pruned_thickness(d2, offsets, census, np.asarray(pruned)[:, :, :6], ['a', 'b'])
    with pytest.raises(ValueError):
        skeleton.build_pruned_thickness(d2, [0, 16, 16, 17, 21], census, pruned, ['a', 'b'])           # lists of the unpruned skeleton
    wrong = np.array(pruned)
    wrong[0, 0, 0] = 15
    with pytest.raises(ValueError, match='input'):
        skeleton.build_pruned_thickness(d2, offsets, census, wrong, ['a', 'b'])


# ---- 6. the command line
def _mask_dir(tmp_path):
    from PIL import Image
    mask_dir = tmp_path / 'masks'
    mask_dir.mkdir()
    cases = K.hand_cases()
    for name, lumen, cap in (('s1.tiff', cases['bar5'][0], cases['bar4'][0]), ('s0.tiff', cases['bar4'][0], np.zeros((9, 24), bool))):
        arr = np.zeros((9, 24, 4), np.uint8)
        arr[:, :, 0] = lumen * 255
        arr[:, :, 1] = cap * 255
        Image.fromarray(arr).save(str(mask_dir / name))
    return mask_dir


def _lists(stack, channels):                                 # what the GPU would return, from the restatements
    out, cen = R.skeleton_stack(stack)
    d2, off, _ = R.width_lists(np.asarray(stack)[..., list(channels)], out[..., list(channels)])
    return d2, off, cen[:, list(channels)]


def _pruned_lists(stack, channels, spur, trim):
    out, cen = R.skeleton_stack(stack)
    cut, pc = P.prune_stack(out, spur, trim)
    d2, off, _ = R.width_lists(np.asarray(stack)[..., list(channels)], cut[..., list(channels)])
    return d2, off, cen[:, list(channels)], pc[:, list(channels)]


def test_main_with_spur_and_trim(tmp_path, monkeypatch):
    mask_dir, save_dir = _mask_dir(tmp_path), tmp_path / 'out'
    monkeypatch.setattr(skeleton, '_host_lists', _lists)
    monkeypatch.setattr(skeleton, '_host_pruned_lists', _pruned_lists)
    report = skeleton.main([str(mask_dir), str(save_dir), 'trim=3', 'spur=2'])
    saved = json.load(open(save_dir / 'medial_thickness.json'))
    assert saved == json.loads(json.dumps(report))
    assert saved['spur'] == 2 and saved['trim'] == 3 and saved['images'] == ['s0.tiff', 's1.tiff']
    lumen, cap = saved['thickness']['Lumen'], saved['thickness']['Fibrous cap']
    # bar4 thins to 17 pixels, bar5 to 16: straight rows, three pixels off either end
    assert lumen['slice'] == [0, 1] and lumen['centreline'] == [11, 10] and lumen['removed'] == [6, 6] and lumen['restored'] == [0, 0]
    assert lumen['tips'] == [2, 2] and lumen['ends'] == [2, 2] and lumen['length'] == [10.0, 9.0] and lumen['passes'] == [2, 2]
    assert lumen['max'] == [3.0, 5.0] and lumen['min'] == [3.0, 5.0]
    assert cap['slice'] == [1] and cap['centreline'] == [11] and saved['thickness']['Lipid core']['slice'] == []
    # longer than the rows: the 17-pixel row shrinks to its middle pixel (an isolated pixel is no tip), the 16-pixel row ends as two facing tips,
    # vanishes in one pass and is restored whole
    big = skeleton.main([str(mask_dir), 'trim=40'])
    assert big['trim'] == 40 and big['spur'] == 0 and big['thickness']['Lumen']['centreline'] == [1, 16]
    assert big['thickness']['Lumen']['restored'] == [0, 16] and os.path.exists(mask_dir / 'medial_thickness.json')
    with pytest.raises(SystemExit):
        skeleton.main(['spur=3'])
    with pytest.raises(SystemExit):
        skeleton.main([str(mask_dir), str(save_dir), 'extra', 'trim=1'])
    with pytest.raises(ValueError, match='0..8192'):
        skeleton.main([str(mask_dir), 'trim=9000'])


def test_main_without_the_new_words_is_unchanged(tmp_path, monkeypatch):
    mask_dir, save_dir = _mask_dir(tmp_path), tmp_path / 'out'
    monkeypatch.setattr(skeleton, '_host_lists', _lists)

    def never(*args):
        raise AssertionError('the pruned lists are not asked for without spur or trim')
    monkeypatch.setattr(skeleton, '_host_pruned_lists', never)
    for argv in ([str(mask_dir), str(save_dir)], [str(mask_dir), str(save_dir), 'spur=0', 'trim=0']):
        report = skeleton.main(argv)
        assert sorted(report) == ['classes', 'images', 'thickness', 'unit', 'width']
        names = ['s0.tiff', 's1.tiff']
        stack = skeleton.read_mask_dir(str(mask_dir))[1]
        d2, off, cen = _lists(stack, range(4))
        want = {'images': names, 'classes': ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum'], 'unit': 'pixel', 'width': '2 * sqrt(d2) - 1',
                'thickness': skeleton.build_thickness(d2, off, cen, ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum'], names=names)}
        assert report == want
        assert open(save_dir / 'medial_thickness.json').read() == json.dumps(want, indent=1)
        assert list(report['thickness']['Lumen']) == ['slice', 'image', 'centreline', 'ends', 'junctions', 'passes', 'median', 'mean', 'min', 'p5',
                                                      'max']
