"""Mask clean-up on the GPU (csrc/components.hip through oct_segmentation_amd/cleanup.py) against the scipy reference of tests/cleanup_ref.py.
Every comparison is integer equality: there is no tolerance in this feature."""
import functools

import numpy as np
import pytest
import torch

import cleanup_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import analysis, cleanup
from cleanup_ref import golden_planes, salt

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 129), (130, 97), (300, 257)]


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded_stack(h, w, n=3):
    """[n, h, w, 4]: channel 0 random at density 0.5, 1 sparse at 0.01, 2 empty, 3 full.  Read-only: shared between tests."""
    rng = np.random.RandomState(1000 * h + w)
    st = np.zeros((n, h, w, 4), np.float32)
    st[..., 0] = rng.rand(n, h, w) < 0.5
    st[..., 1] = rng.rand(n, h, w) < 0.01
    st[..., 3] = 1.0
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def ref_labels(h, w):
    return R.label_stack(seeded_stack(h, w))


@functools.lru_cache(maxsize=None)
def ref_table(h, w):
    return R.table_stack(seeded_stack(h, w))


def plane_stack(*planes):
    """[1, H, W, len(planes)] from 2-D planes."""
    return np.stack([np.asarray(p, np.float32) for p in planes], axis=-1)[None]


# ---- patterns that break merges
def spiral(h, w):
    """A one-pixel-wide arm wound inwards with one-pixel gaps: a single component, the longest chain of unions."""
    m = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ny2 < h and 0 <= nx2 < w and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return (yy + xx) % 2 == 0


def pixel_grid(h, w):
    yy, xx = np.mgrid[:h, :w]
    return (yy % 2 == 0) & (xx % 2 == 0)


def diagonal_blobs(h, w):
    """Two blobs that touch only diagonally where a 64-pixel row word ends: (63, 63) and (64, 64); a second pair the other way round."""
    m = np.zeros((h, w), bool)
    m[58:64, 58:64] = True
    m[64:70, 64:70] = True
    m[20:26, 64:70] = True
    m[26:32, 58:64] = True
    return m


def border_ring(h, w):
    """A ring whose opening lies on the frame border: its inside is connected to the outside, not a hole."""
    m = np.zeros((h, w), bool)
    m[0:30, 50:80] = True
    m[0:26, 54:76] = False
    m[h - 20:h, 0:25] = True
    m[h - 16:h - 4, 0:21] = False          # the opening on the left border
    return m


def ring_with_island(h, w):
    m = np.zeros((h, w), bool)
    m[10:60, 40:90] = True
    m[14:56, 44:86] = False
    m[30:40, 60:70] = True
    m[33:36, 63:66] = False                 # the island has a hole of its own
    return m


PATTERNS = {'spiral': spiral, 'checkerboard': checkerboard, 'pixel_grid': pixel_grid, 'diagonal_blobs': diagonal_blobs,
            'border_ring': border_ring, 'ring_with_island': ring_with_island}


# ---- 1. labels
@pytest.mark.parametrize('h,w', SHAPES)
def test_labels_equal_the_reference(h, w):
    st = seeded_stack(h, w)
    got = cleanup.label_stack(dev(st))
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 4, h, w)
    assert np.array_equal(host(got), ref_labels(h, w))


# ---- 2. patterns
@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('name', sorted(PATTERNS))
def test_patterns_that_break_merges(name, transposed):
    h, w = (97, 130) if transposed else (130, 97)
    m = PATTERNS[name](w, h).T if transposed else PATTERNS[name](h, w)
    assert m.shape == (h, w)
    st = plane_stack(m)
    want_n, want_top = R.table_stack(st)
    if name in ('spiral', 'checkerboard'):
        assert want_n[0, 0] == 1
    if name == 'pixel_grid':
        assert want_n[0, 0] == ((h + 1) // 2) * ((w + 1) // 2)          # the most components a plane can hold
    if name == 'diagonal_blobs':
        assert want_n[0, 0] == 2
    d = dev(st)
    assert np.array_equal(host(cleanup.label_stack(d)), R.label_stack(st))
    n, top = cleanup.component_table(d)
    assert np.array_equal(host(n), want_n) and np.array_equal(host(top), want_top)
    for fill in (False, True):
        want = R.per_plane(st, lambda p: R.keep_largest(p, 0, 0, fill))
        assert np.array_equal(host(cleanup.keep_largest(d, keep=0, fill_holes=fill)), want)
    filled = host(cleanup.keep_largest(d, keep=0, fill_holes=True))[0, :, :, 0]
    if name == 'border_ring':
        assert np.array_equal(filled, m)                               # nothing to fill
    if name == 'ring_with_island':
        assert filled.sum() == 50 * 50 and m.sum() < 50 * 50


def test_checkerboard_fill_sets_the_interior_background_only():
    m = checkerboard(37, 53)
    assert int((~m).sum()) == 980                                       # 980 separate 4-connected background pixels
    st = plane_stack(m)
    filled = host(cleanup.keep_largest(dev(st), keep=0, fill_holes=True))[0, :, :, 0].astype(bool)
    assert int(filled.sum() - m.sum()) == 892
    inner = np.zeros_like(m)
    inner[1:-1, 1:-1] = True
    assert filled[inner].all() and np.array_equal(filled[~inner], m[~inner])   # the border's background pixels stay


# ---- 3. tables
@pytest.mark.parametrize('h,w', [(37, 53), (65, 129), (130, 97)])
def test_tables_equal_the_reference(h, w):
    n, top = cleanup.component_table(dev(seeded_stack(h, w)))
    want_n, want_top = ref_table(h, w)
    assert n.dtype == torch.int32 and top.dtype == torch.int32 and tuple(top.shape) == (3, 4, 8, 6)
    assert np.array_equal(host(n), want_n) and np.array_equal(host(top), want_top)
    assert want_n[:, 0].min() > 8 and (want_n[:, 2] == 0).all() and (want_n[:, 3] == 1).all()


def tie_plane():
    """Eleven boxes: seven of distinct areas, then four of area 6 -- rows 8 and 9 of the ranking tie, the first pixel decides who is listed."""
    m = np.zeros((40, 100), bool)
    for i in range(7):
        m[0:3 + i, 8 * i:8 * i + 5] = True                             # areas 15, 20, ... 45
    for x in (90, 70, 80, 60):
        m[30:32, x:x + 3] = True
    return m


def test_table_tie_break_at_rows_eight_and_nine():
    st = plane_stack(tie_plane(), tie_plane()[::-1].copy())
    want_n, want_top = R.table_stack(st)
    assert want_n.tolist() == [[11, 11]] and want_top[0, 0, 7].tolist() == [6, 30 * 100 + 60, 60, 30, 62, 31]
    n, top = cleanup.component_table(dev(st))
    assert np.array_equal(host(n), want_n) and np.array_equal(host(top), want_top)


# ---- 4. keep_largest
@pytest.mark.parametrize('fill', [False, True])
@pytest.mark.parametrize('keep,min_area', [(1, 0), (3, 0), (100, 0), (0, 5), (9, 0), (12, 3)])
def test_keep_largest(keep, min_area, fill):
    for h, w in ((37, 53), (130, 97)):
        st = seeded_stack(h, w)
        want = R.per_plane(st, lambda p: R.keep_largest(p, keep, min_area, fill))
        got = cleanup.keep_largest(dev(st), keep=keep, min_area=min_area, fill_holes=fill)
        assert got.dtype == torch.float32 and got.shape == st.shape
        assert np.array_equal(host(got), want)


@pytest.mark.parametrize('fill', [False, True])
def test_keep_largest_four_way_tie_at_the_threshold(fill):
    m = np.zeros((40, 100), bool)
    m[2:12, 2:12] = True
    m[4:8, 4:8] = False                                                 # a hole in the largest
    for x in (20, 40, 60, 80):
        m[20:23, x:x + 3] = True                                        # four of area 9
    m[35, 50] = True
    st = plane_stack(m)
    got = host(cleanup.keep_largest(dev(st), keep=2, fill_holes=fill))
    assert np.array_equal(got, R.per_plane(st, lambda p: R.keep_largest(p, 2, 0, fill)))
    assert got.sum() == 84 + 36 + (16 if fill else 0)                   # the largest and all four of the tie; the speck goes
    out, (n, top) = cleanup.clean_stack(dev(st), smooth=False, keep=2, fill_holes=fill, return_table=True)
    want_n, want_top = R.table_stack(st, lambda p: R.kept_table(p, 2, 0))
    assert host(n).tolist() == [[5]] and np.array_equal(host(n), want_n) and np.array_equal(host(top), want_top)


# ---- 5. smoothing
def border_blobs(h, w, seed):
    rng = np.random.RandomState(seed)
    m = rng.rand(h, w) < 0.35
    m[0:6, 0:7] = True
    m[h - 7:h, w - 6:w] = True
    m[0:5, w - 9:w] = True
    m[h // 2 - 4:h // 2 + 4, 0:6] = True
    return m


@pytest.mark.parametrize('k', range(1, 8))
def test_smooth_stack(k):
    for h, w in ((37, 53), (130, 97)):
        st = np.concatenate([seeded_stack(h, w)[:1], plane_stack(border_blobs(h, w, 1), border_blobs(h, w, 2), border_blobs(h, w, 3) * 0,
                                                                 np.ones((h, w)))])
        want = R.per_plane(st, lambda p: R.smooth(p, k))
        got = host(cleanup.smooth_stack(dev(st), kernel_size=k))
        assert np.array_equal(got, want)
        assert got[1, 0, 0, 0] == 1 and got[1, h - 1, w - 1, 0] == 1 and got[1, 0, w - 1, 0] == 1 and got[1, h // 2, 0, 0] == 1   # border, corners
        if k == 1:
            assert np.array_equal(got, (st != 0).astype(np.float32))


@pytest.mark.parametrize('h,w,k', [(400, 600, 2), (750, 750, 3)])
def test_smooth_stack_picks_the_reference_size(h, w, k):
    assert cleanup.smooth_kernel_size(h, w) == k
    st = plane_stack(border_blobs(h, w, k))
    got = host(cleanup.smooth_stack(dev(st)))
    assert np.array_equal(got, R.per_plane(st, lambda p: R.smooth(p, k)))
    assert not np.array_equal(got, R.per_plane(st, lambda p: R.smooth(p, k + 1)))


def test_smooth_stack_refuses_size_eight():
    d = dev(seeded_stack(37, 53))
    with pytest.raises(ValueError):
        cleanup.smooth_stack(d, kernel_size=8)
    with pytest.raises(ValueError):
        cleanup.smooth_stack(torch.zeros((1, 1600, 1600, 1), device='cuda'))          # the reference's rule asks for 8 here


# ---- 6. the chain, chunked
def test_clean_stack_chain_and_chunks():
    h, w = 130, 97
    st = seeded_stack(h, w)
    d = dev(st)
    want = R.per_plane(st, lambda p: R.clean(p, 3, 3, 2, True))
    want_n, want_top = R.table_stack(st, lambda p: R.kept_table(R.smooth(p, 3), 3, 2))
    one, (n, top) = cleanup.clean_stack(d, smooth=3, keep=3, min_area=2, return_table=True)
    assert np.array_equal(host(one), want) and np.array_equal(host(n), want_n) and np.array_equal(host(top), want_top)
    lib = L.lib()
    per_plane, per_slice = lib.octseg_components_scratch_bytes(1, h, w), lib.octseg_components_scratch_bytes(4, h, w)
    for budget in (per_plane, per_slice, 2 * per_slice + 1):
        out, (n2, top2) = cleanup.clean_stack(d, smooth=3, keep=3, min_area=2, return_table=True, scratch_bytes=budget)
        assert torch.equal(out, one) and torch.equal(n2, n) and torch.equal(top2, top), budget
    # the defaults: the reference's size rule gives 1 at this frame size (no smoothing), keep 3, fill
    assert np.array_equal(host(cleanup.clean_stack(d)), R.per_plane(st, lambda p: R.clean(p, None, 3, 0, True)))


# ---- 7. goldens
@functools.lru_cache(maxsize=None)
def golden_stacks():
    """([6, 750, 750, 4] clean, the same with seeded salt noise on every channel): plane i of the fixture sits in its own channel of slice i."""
    planes, slices, channels, _, _ = golden_planes()
    st = np.zeros((len(planes), 750, 750, 4), np.float32)
    for i, c in enumerate(channels):
        st[i, :, :, c] = planes[i]
    noisy = np.maximum(st, salt(st.shape, 2024).astype(np.float32))
    st.setflags(write=False)
    noisy.setflags(write=False)
    return st, noisy


@pytest.mark.parametrize('noise', [False, True])
def test_golden_planes(noise):
    st = golden_stacks()[1 if noise else 0]
    want = R.per_plane(st, lambda p: R.clean(p))                        # 750 x 750: the smoothing ellipse is 3
    d = dev(st)
    got = cleanup.clean_stack(d)
    assert np.array_equal(host(got), want)
    # measurements of the cleaned stack: slice 3 / channel 3 is the Vasa vasorum plane of file 129
    c1, r1 = analysis.measure_stack(got)
    c2, r2 = analysis.measure_stack(dev(want))
    assert torch.equal(c1, c2) and torch.equal(r1, r2)
    if noise:
        raw = analysis.measure_stack(d)[0]
        assert int(raw[3, 2]) > 0 and int(c1[3, 2]) == int(want[3, :, :, 2].sum())     # an empty class is "present" through its specks before
    assert analysis.analyze_stack(d, clean=True) == analysis.analyze_stack(got)
    assert analysis.analyze_stack(d, clean={'smooth': False, 'keep': 1}) == analysis.analyze_stack(cleanup.clean_stack(d, smooth=False, keep=1))


# ---- 8. MaskProcessor
def test_mask_processor_on_numpy_input():
    planes = golden_planes()[0]
    noisy = (planes[3] | salt(planes[3].shape, 129)).astype(np.uint8) * 255
    mp = cleanup.MaskProcessor()
    got = mp.smooth_mask(noisy)
    assert got.dtype == np.uint8 and got.shape == noisy.shape and np.array_equal(got, R.smooth(noisy))
    got = mp.remove_artifacts(noisy)
    assert got.dtype == np.uint8 and np.array_equal(got, R.keep_largest(noisy, 3, 0, True))
    assert (got.astype(bool) & planes[3]).sum() == planes[3].sum() == 1430
    small = (np.random.RandomState(5).rand(37, 53) < 0.4).astype(np.uint8)
    assert np.array_equal(cleanup.MaskProcessor.remove_artifacts(small), R.keep_largest(small, 3, 0, True))
    assert np.array_equal(cleanup.MaskProcessor.smooth_mask(small), small)            # k = 1 below 400 pixels


# ---- 9. sentinels
def test_outputs_stay_inside_their_extent_and_refused_calls_launch_nothing():
    h, w = 65, 129
    st = seeded_stack(h, w)
    d = dev(st)
    before = d.clone()
    lib = L.lib()
    need = int(lib.octseg_components_scratch_bytes(12, h, w))
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    labels = torch.full((13, h, w), 7, dtype=torch.int32, device='cuda')
    ncomp = torch.full((13,), 7, dtype=torch.int32, device='cuda')
    top = torch.full((13, 8, 6), 7, dtype=torch.int32, device='cuda')
    out = torch.full((4, h, w, 4), 7.0, dtype=torch.float32, device='cuda')
    s = L.stream_ptr()
    # refused calls first: nothing may be written
    assert lib.octseg_stack_components(L.ptr(d), 3, h, w, 4, None, need, L.ptr(labels), L.ptr(ncomp), L.ptr(top), s) == -5
    assert lib.octseg_stack_components(L.ptr(d), 3, h, w, 4, L.ptr(scratch), need - 1, L.ptr(labels), L.ptr(ncomp), L.ptr(top), s) == -5
    assert lib.octseg_stack_components(L.ptr(d), 3, 0, w, 4, L.ptr(scratch), need, L.ptr(labels), L.ptr(ncomp), L.ptr(top), s) == -1
    assert lib.octseg_stack_cleanup(L.ptr(d), 3, h, w, 4, 8, 3, 0, 1, L.ptr(scratch), need, L.ptr(out), L.ptr(ncomp), L.ptr(top), s) == -1
    assert lib.octseg_stack_cleanup(L.ptr(d), 3, h, w, 17, 3, 3, 0, 1, L.ptr(scratch), need, L.ptr(out), L.ptr(ncomp), L.ptr(top), s) == -1
    assert lib.octseg_stack_cleanup(L.ptr(d), 3, h, w, 4, 3, 3, 0, 1, L.ptr(scratch), need, None, L.ptr(ncomp), L.ptr(top), s) == -5
    torch.cuda.synchronize()
    assert (labels == 7).all() and (ncomp == 7).all() and (top == 7).all() and (out == 7).all()
    L.check(lib.octseg_stack_components(L.ptr(d), 3, h, w, 4, L.ptr(scratch), need, L.ptr(labels), L.ptr(ncomp), L.ptr(top), s))
    assert np.array_equal(host(labels[:12]).reshape(3, 4, h, w), ref_labels(h, w))
    assert (labels[12] == 7).all() and (ncomp[12] == 7).all() and (top[12] == 7).all()
    assert np.array_equal(host(ncomp[:12]).reshape(3, 4), ref_table(h, w)[0]) and np.array_equal(host(top[:12]).reshape(3, 4, 8, 6), ref_table(h, w)[1])
    ncomp.fill_(7)
    top.fill_(7)
    L.check(lib.octseg_stack_cleanup(L.ptr(d), 3, h, w, 4, 2, 3, 0, 1, L.ptr(scratch), need, L.ptr(out), L.ptr(ncomp), L.ptr(top), s))
    assert np.array_equal(host(out[:3]), R.per_plane(st, lambda p: R.clean(p, 2, 3, 0, True)))
    assert (out[3] == 7).all() and (ncomp[12] == 7).all() and (top[12] == 7).all()
    want_n, want_top = R.table_stack(st, lambda p: R.kept_table(R.smooth(p, 2), 3, 0))
    assert np.array_equal(host(ncomp[:12]).reshape(3, 4), want_n) and np.array_equal(host(top[:12]).reshape(3, 4, 8, 6), want_top)
    assert torch.equal(d, before)                                       # the input stack is never modified
    for fn in (cleanup.label_stack, cleanup.component_table, cleanup.smooth_stack, cleanup.keep_largest, cleanup.clean_stack):
        fn(d)
    assert torch.equal(d, before)


# ---- 10. the scratch is work space only: no result depends on what it held (the labelling initialises its counters at run starts only)
SCRATCH_FILLS = (0x00, 0xFF, 0x55)


@functools.lru_cache(maxsize=None)
def density_stack(ch):
    """[2, 9, 65, ch]: seeded random planes at densities 0.45 / 0.03 / 0.9 (/ 0.45); W crosses one word boundary.  Read-only."""
    rng = np.random.RandomState(965 + ch)
    st = np.stack([rng.rand(2, 9, 65) < p for p in (0.45, 0.03, 0.9, 0.45)[:ch]], axis=-1).astype(np.float32)
    st.setflags(write=False)
    return st


@pytest.mark.parametrize('ch', [3, 4])                                  # the scalar pack / unpack path, the float4 one
def test_stack_cleanup_does_not_depend_on_the_scratch(ch):
    st = density_stack(ch)
    n, h, w, _ = st.shape
    d = dev(st)
    lib = L.lib()
    need = int(lib.octseg_components_scratch_bytes(n * ch, h, w))
    got = []
    for fill in SCRATCH_FILLS:
        scratch = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        out = torch.full((n, h, w, ch), 7.0, dtype=torch.float32, device='cuda')
        ncomp = torch.full((n * ch,), 7, dtype=torch.int32, device='cuda')
        top = torch.full((n * ch, 8, 6), 7, dtype=torch.int32, device='cuda')
        # smoothing, the labelling with the filter, and the labelling of the complement for the fill: two labelling passes over one scratch
        L.check(lib.octseg_stack_cleanup(L.ptr(d), n, h, w, ch, 2, 3, 2, 1, L.ptr(scratch), need, L.ptr(out), L.ptr(ncomp), L.ptr(top),
                                         L.stream_ptr()))
        got.append((host(out), host(ncomp).reshape(n, ch), host(top).reshape(n, ch, 8, 6)))
    want_n, want_top = R.table_stack(st, lambda p: R.kept_table(R.smooth(p, 2), 3, 2))
    want = (R.per_plane(st, lambda p: R.clean(p, 2, 3, 2, True)), want_n, want_top)
    for fill, g in zip(SCRATCH_FILLS, got):
        for name, a, b, first in zip(('out', 'ncomp', 'top'), g, want, got[0]):
            assert np.array_equal(a, first), f'{name} differs between scratch fills 0x00 and {fill:#04x}'
            assert np.array_equal(a, b), f'{name} differs from the reference with scratch fill {fill:#04x}'


def test_stack_components_do_not_depend_on_the_scratch():
    st = density_stack(3)
    n, h, w, ch = st.shape
    d = dev(st)
    lib = L.lib()
    need = int(lib.octseg_components_scratch_bytes(n * ch, h, w))
    got = []
    for fill in SCRATCH_FILLS:
        scratch = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        labels = torch.full((n * ch, h, w), 7, dtype=torch.int32, device='cuda')
        ncomp = torch.full((n * ch,), 7, dtype=torch.int32, device='cuda')
        top = torch.full((n * ch, 8, 6), 7, dtype=torch.int32, device='cuda')
        L.check(lib.octseg_stack_components(L.ptr(d), n, h, w, ch, L.ptr(scratch), need, L.ptr(labels), L.ptr(ncomp), L.ptr(top), L.stream_ptr()))
        got.append((host(labels).reshape(n, ch, h, w), host(ncomp).reshape(n, ch), host(top).reshape(n, ch, 8, 6)))
    want = (R.label_stack(st),) + R.table_stack(st)
    for fill, g in zip(SCRATCH_FILLS, got):
        for name, a, b, first in zip(('labels', 'ncomp', 'top'), g, want, got[0]):
            assert np.array_equal(a, first), f'{name} differs between scratch fills 0x00 and {fill:#04x}'
            assert np.array_equal(a, b), f'{name} differs from the reference with scratch fill {fill:#04x}'


def test_wrappers_refuse_wrong_dtype_rank_and_channels():
    for bad in (torch.zeros((1, 4, 4, 4), dtype=torch.float64, device='cuda'), torch.zeros((4, 4, 4), device='cuda'),
                torch.zeros((1, 0, 4, 4), device='cuda'), torch.zeros((1, 4, 4, 17), device='cuda')):
        for fn in (cleanup.label_stack, cleanup.component_table, cleanup.clean_stack):
            with pytest.raises(ValueError):
                fn(bad)
