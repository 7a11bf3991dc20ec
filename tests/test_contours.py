"""Mask outlines without a GPU: the sequential crack follower of tests/contours_ref.py (the restatement the kernels are held to) proven against
scipy.ndimage.label and matplotlib.path on every case the GPU test uses; the host half of oct_segmentation_amd/contours.py (polygons, shapes, report,
SVG) on a Contours built from the reference; the ABI's declarations and refusals."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch
from matplotlib.path import Path
from scipy import ndimage

import contours_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import contours

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 129), (130, 97), (300, 257)]
FULL = np.ones((3, 3), int)


def planes_of(h, w):
    st = R.seeded_stack(h, w, channels=(0.01, 1.0) if (h, w) == (300, 257) else (0.5, 0.01, 0.0, 1.0))
    return [st[i, :, :, c] != 0 for i in range(st.shape[0]) for c in range(st.shape[3])]


def check_plane(m):
    """Every invariant of the issue on one plane."""
    h, w = m.shape
    conts = R.trace_plane(m)
    outer, holes = [c for c in conts if c['area'] > 0], [c for c in conts if c['area'] < 0]
    assert len(outer) + len(holes) == len(conts)
    lab8, n8 = ndimage.label(m, structure=FULL)
    assert len(outer) == n8                                                       # outer contours = 8-connected components
    ring = np.zeros((h + 2, w + 2), bool)
    ring[1:-1, 1:-1] = m
    lab4, n4 = ndimage.label(~ring)                                               # 4-connected complement, padded by a clear ring
    assert len(holes) == n4 - 1                                                   # ... minus the outside
    assert sum(c['area'] for c in conts) == int(m.sum())
    assert [c['leader'] for c in conts] == sorted(c['leader'] for c in conts)     # leader order
    first = {}
    for k in range(1, n8 + 1):
        first[k] = int(np.flatnonzero((lab8 == k).ravel())[0])
    for c in outer:
        d, x, y = c['leader'] & 3, (c['leader'] >> 2) % (w + 1), (c['leader'] >> 2) // (w + 1)
        assert d == 0 and c['ring'][0] == [x, y]
        k = lab8[y, x]
        assert k > 0 and first[k] == y * w + x and c['label'] == 1 + y * w + x     # the leader pixel is the component's first raster pixel
        assert c['area'] == int(ndimage.binary_fill_holes(lab8 == k).sum())
    for c in holes:
        d, x, y = c['leader'] & 3, (c['leader'] >> 2) % (w + 1), (c['leader'] >> 2) // (w + 1)
        assert d == 1 and c['ring'][0] == [x, y]
        assert m[y, x - 1] and not m[y, x]                                        # the enclosing component's pixel beside the hole's first pixel
        assert c['label'] == 1 + first[lab8[y, x - 1]]
        # minus the hole's pixels, the islands inside it counted in (they are contours of their own and add their pixels back): the hole is
        # 4-connected, so what it encloses is what the frame's border does not reach through its 8-connected complement
        assert -c['area'] == int(ndimage.binary_fill_holes(lab4 == lab4[y + 1, x + 1], structure=FULL).sum())
    for c in conts:
        assert c['vertices'] % 2 == 0 and c['vertices'] >= 4
        r = np.asarray(c['ring'])
        nxt = np.roll(r, -1, axis=0)
        assert int((r[:, 0] * nxt[:, 1] - nxt[:, 0] * r[:, 1]).sum()) == 2 * c['area']                # the shoelace formula over the vertex list
        assert int(np.abs(nxt - r).sum()) == c['edges']                                               # axis-parallel sides: the crack perimeter
        assert (c['x0'], c['y0'], c['x1'], c['y1']) == (r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max())
    assert np.array_equal(even_odd_fill([c['ring'] for c in conts], h, w), m)
    return conts


def even_odd_fill(rings, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    pts = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], axis=1)
    out = np.zeros(h * w, bool)
    for ring in rings:
        out ^= Path(np.asarray(ring, float)).contains_points(pts)
    return out.reshape(h, w)


@pytest.mark.parametrize('h,w', SHAPES)
def test_reference_on_the_seeded_stacks(h, w):
    for m in planes_of(h, w):
        check_plane(m)


@pytest.mark.parametrize('name', sorted(R.patterns()))
def test_reference_on_the_patterns(name):
    m = R.patterns()[name]
    conts = check_plane(m)
    if name == 'checkerboard':
        assert len(conts) == 32 and sum(c['vertices'] for c in conts) == 200
    if name == 'staircase':
        assert len(conts) == 1 and conts[0]['vertices'] == conts[0]['edges'] == 4 * 23                  # through every ambiguous vertex
    if name == 'rings':
        assert [c['area'] for c in conts] == [144, -64, 16] and [c['label'] for c in conts] == [1, 1, 1 + 4 * 12 + 4]
    if name == 'spiral':
        assert len(conts) == 1 and conts[0]['edges'] > 8192
    if name.startswith(('bar', 'column')):
        n = int(''.join(ch for ch in name if ch.isdigit()))
        assert len(conts) == 1 and conts[0]['edges'] == 2 * n + 2 and conts[0]['vertices'] == 4
    if name == 'frame_blobs':
        assert len(conts) == 2 and (min(c['x0'] for c in conts), min(c['y0'] for c in conts)) == (0, 0)
        assert (max(c['x1'] for c in conts), max(c['y1'] for c in conts)) == (70, 40)
    if name == 'hole_at_checker_vertex':
        assert [c['area'] for c in conts] == [64, -1, -7] and conts[2]['ring'][0] == [3, 3] and conts[1]['ring'][0] == [2, 2]


def test_counts_are_local():
    """The two counts need no tracing: edges are (set, clear) 4-neighbour pairs, vertices come from the 2 x 2 neighbourhoods."""
    for m in planes_of(37, 53) + list(R.patterns().values()):
        counts = R.trace_stack(np.asarray(m, np.float32)[None, :, :, None])[3][0, 0]
        p = np.pad(m, 1)
        edges = sum(int((p[1:-1, 1:-1] & ~np.roll(p, s, axis=a)[1:-1, 1:-1]).sum()) for s, a in ((1, 0), (-1, 0), (1, 1), (-1, 1)))
        q = p[:-1, :-1].astype(int) + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:]
        diag = (p[:-1, :-1] == p[1:, 1:]) & (p[:-1, 1:] == p[1:, :-1]) & (p[:-1, :-1] != p[:-1, 1:])
        assert counts[0] == edges and counts[1] == int((q % 2 == 1).sum() + 2 * diag.sum())


# ---- the host half of the module on a Contours built from the reference
@functools.lru_cache(maxsize=None)
def demo():
    st = np.zeros((2, 12, 14, 4), np.float32)
    st[0, :, :12, 0] = R.patterns()['rings']
    st[0, 2:5, 3:9, 1] = 1
    st[1, 1:11, 1:11, 3] = R.patterns()['hole_at_checker_vertex']
    st[1, 0, 13, 3] = 1
    ncont, table, verts, _ = R.trace_stack(st)
    return st, contours.Contours(ncont, table, verts, (14, 12))


def test_polygons_and_shapes():
    st, cont = demo()
    polys = cont.polygons()
    assert len(polys) == 2 and all(len(f) == 4 for f in polys)
    ring, island = polys[0][0]
    assert ring['label'] == 1 and ring['holes'] == 1 and ring['area'] == 144 - 64 and ring['perimeter'] == 48 + 32 and ring['bbox'] == [0, 0, 12, 12]
    assert ring['exterior'] == [[0, 0], [12, 0], [12, 12], [0, 12]] and ring['interior'] == [[[2, 2], [2, 10], [10, 10], [10, 2]]]
    assert island == {'label': 1 + 4 * 14 + 4, 'exterior': [[4, 4], [8, 4], [8, 8], [4, 8]], 'interior': [], 'area': 16, 'perimeter': 16, 'holes': 0,
                      'bbox': [4, 4, 8, 8]}
    assert polys[0][1][0]['area'] == 18 and polys[0][2] == [] and polys[1][0] == []
    blob, speck = sorted(polys[1][3], key=lambda p: -p['area'])
    assert blob['holes'] == 2 and blob['area'] == 64 - 8 and speck['area'] == 1 and speck['exterior'] == [[13, 0], [14, 0], [14, 1], [13, 1]]
    for i in range(2):
        for c in range(4):
            rings = [r for p in polys[i][c] for r in [p['exterior']] + p['interior']]
            assert np.array_equal(even_odd_fill(rings, 12, 14), st[i, :, :, c] != 0)
            lab, n = ndimage.label(st[i, :, :, c], structure=FULL)
            assert sorted(p['area'] for p in polys[i][c]) == sorted(int((lab == k).sum()) for k in range(1, n + 1))
    shapes = contours.component_shapes(cont)
    assert shapes[0][0] == [{'label': 1, 'area': 80, 'perimeter': 80, 'holes': 1, 'euler': 0, 'bbox': [0, 0, 12, 12]},
                            {'label': 61, 'area': 16, 'perimeter': 16, 'holes': 0, 'euler': 1, 'bbox': [4, 4, 8, 8]}]
    assert [s['euler'] for s in shapes[1][3]] == [-1, 1] and [s['area'] for s in shapes[1][3]] == [56, 1]


def test_report_and_svg():
    st, cont = demo()
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    rep = contours.contour_report(cont, ['a', 'b'], names)
    assert json.loads(json.dumps(rep)) == rep
    assert rep['convention'] == contours.CONVENTION and 'x + 0.5' in rep['convention'] and 'not cv2.findContours' in rep['convention']
    assert (rep['width'], rep['height'], rep['classes']) == (14, 12, names) and [s['name'] for s in rep['slices']] == ['a', 'b']
    assert rep['slices'][0]['objects']['Lumen'] == cont.polygons()[0][0] and rep['slices'][1]['objects']['Lumen'] == []
    assert contours.contour_report(cont)['classes'] == names and [s['name'] for s in contours.contour_report(cont)['slices']] == ['0', '1']
    with pytest.raises(ValueError):
        contours.contour_report(cont, ['a'])
    with pytest.raises(ValueError):
        contours.contour_report(cont, None, names[:3])
    svg = contours.svg_frame(cont.polygons()[0], (14, 12), names)
    paths = re.findall(r'<path id="([^"]+)" fill="(#[0-9a-f]{6})"[^>]*fill-rule="evenodd" d="([^"]*)"/>', svg)
    assert [p[0] for p in paths] == names and svg.startswith('<svg ') and 'viewBox="0 0 14 12"' in svg
    assert paths[0][1] == '#e41ec7' and paths[3][1] == '#d0021b'                                           # the class colours of the overlays
    assert paths[0][2] == 'M 0 0 L 12 0 L 12 12 L 0 12 Z M 2 2 L 2 10 L 10 10 L 10 2 Z M 4 4 L 8 4 L 8 8 L 4 8 Z' and paths[2][2] == ''
    with pytest.raises(ValueError):
        contours.svg_frame(cont.polygons()[0], (14, 12), names[:2])


def test_wrappers_refuse_host_tensors():
    for fn in (contours.count_stack, contours.trace_stack, contours.component_shapes, contours.contour_report):
        with pytest.raises(ValueError):
            fn(torch.zeros((1, 4, 4, 4)))
        with pytest.raises(ValueError):
            fn(np.zeros((1, 4, 4, 4), np.float32))


# ---- the ABI
def test_library_exports_the_new_symbols_with_the_declared_signatures():
    lib = L.lib()
    _P = C.c_void_p
    want = {'octseg_stack_contour_counts': (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P]),
            'octseg_contours_scratch_bytes': (C.c_size_t, [C.c_int] * 3 + [C.c_longlong]),
            'octseg_stack_contours': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t] + [C.c_longlong] * 3 + [_P] * 5)}
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert L.SYMBOLS[name] == (res, args)
        assert f'{name}(' in header
    assert f'#define OCTSEG_CONTOUR_FIELDS {contours.NFIELDS}' in header and contours.FIELDS == R.FIELDS
    assert '#define OCTSEG_CONTOUR_MAX_VERTICES (1 << 29)' in header and contours.MAX_VERTICES == 1 << 29


def test_abi_argument_checks_need_no_gpu():
    """Every refusal returns its code with a null stream: it happens before any HIP call, so nothing is launched (there is no GPU here to launch on)."""
    lib = L.lib()
    one = 8      # any non-null, 8-byte aligned pointer value
    big = 1 << 40
    sb = lib.octseg_contours_scratch_bytes
    assert sb(0, 4, 4, 10) == 0 and sb(1, 0, 4, 10) == 0 and sb(1, 4, -1, 10) == 0 and sb(1, 4, 4, 0) == 0 and sb(1, 4, 4, 1 << 31) == 0
    assert sb(1, 1 << 16, 1 << 15, 10) == 0                                         # H * W = 2^31
    assert sb(1, 1 << 15, 1 << 14, 10) == 0 and sb(1, 23000, 23000, 10) > 0         # (H + 1) * (W + 1) >= 2^29: an edge id would not fit 31 bits
    assert sb(1 << 30, 4, 4, 10) == 0                                               # 2^30 planes of 5 vertex words: not below 2^31
    al = lambda v: (v + 255) // 256 * 256                                           # noqa: E731
    # bit planes, parent, vertex-word offsets; per edge: predecessor, id, two jump nodes, (contour, base), order, vertex position; tile sums; scalars
    assert sb(2, 5, 70, 100) == (al(2 * 5 * 2 * 8) + al(2 * 350 * 4) + al(2 * 6 * 2 * 4) + 2 * al(400) + 2 * al(1600) + al(800) + 2 * al(400)
                                 + al(2 * 8) + al(8 * 4))
    assert sb(2, 5, 70, 101) > sb(2, 5, 70, 100) - 1 and sb(3, 5, 70, 100) > sb(2, 5, 70, 100)

    def counts(stack=one, N=1, H=4, W=4, ch=4, out=one):
        return lib.octseg_stack_contour_counts(stack, N, H, W, ch, out, None)

    def trace(stack=one, N=1, H=4, W=4, ch=4, scratch=one, nbytes=big, ecap=64, ccap=16, vcap=64, ncont=one, table=one, verts=one, overflow=one):
        return lib.octseg_stack_contours(stack, N, H, W, ch, scratch, nbytes, ecap, ccap, vcap, ncont, table, verts, overflow, None)

    for call in (counts, trace):
        assert call(stack=None) == -5
        for kw in ({'N': 0}, {'H': 0}, {'W': -1}, {'ch': 0}, {'ch': 17}, {'H': 1 << 16, 'W': 1 << 15}, {'H': 1 << 15, 'W': 1 << 14}):
            assert call(**kw) == -1, kw
    assert counts(out=None) == -5 and counts(out=12) == -5
    assert b'8-byte' in lib.octseg_last_error()
    for name in ('scratch', 'ncont', 'table', 'verts', 'overflow'):
        assert trace(**{name: None}) == -5, name
    assert trace(scratch=12) == -5
    assert trace(nbytes=sb(4, 4, 4, 64) - 1) == -5
    for name in ('ecap', 'ccap', 'vcap'):
        for bad in (0, -1, 1 << 31, 1 << 40):
            assert trace(**{name: bad}) == -5, (name, bad)
    assert b'capacity' in lib.octseg_last_error()
