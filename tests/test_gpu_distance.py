"""Boundary distances on the GPU (csrc/distance.hip through oct_segmentation_amd/distance.py) against the numpy restatement of
tests/distance_ref.py, which tests/test_distance.py holds to scipy.ndimage.  Every comparison is integer equality: there is no tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

import distance_ref as R
from analysis_ref import load_fixture
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 130)]
PARTS = ('set', 'clear', 'boundary')
# (source channel, target channel) over the five channels of seeded_stack: sparse, denser, dense, empty, full -- an empty query, an empty
# target, and a plane against itself are all among them
PAIRS = [(0, 1), (1, 0), (2, 2), (3, 2), (2, 3), (4, 4), (2, 4), (1, 2)]
FIXTURE = os.path.join(os.path.dirname(__file__), 'golden', 'pullback_demo_excerpt.npz')


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded_stack(h, w, n=3):
    """[n, h, w, 5]: densities 0.001, 0.02, 0.5 (one pixel forced into an empty draw), an empty and a full channel.  Read-only."""
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
def ref_maps(h, w):
    st = seeded_stack(h, w)
    return {p: R.distance_stack(st, p) for p in PARTS}, R.boundary_stack(st)


@functools.lru_cache(maxsize=None)
def ref_lists(h, w, src_part, dst_part):
    st = seeded_stack(h, w)
    return R.directed(st, st, PAIRS, src_part, dst_part), R.pair_min(st, st, PAIRS, src_part, dst_part), R.overlap(st, st, PAIRS)


def misaligned(a):
    """The stack as a contiguous CUDA view whose base is 4 bytes off 16-byte alignment."""
    flat = torch.empty((a.size + 1,), dtype=torch.float32, device='cuda')
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def lists_equal(got, want):
    (d2, off, tc), (wd2, woff, wtc) = got, want
    return d2.dtype == np.int64 and np.array_equal(d2, wd2) and np.array_equal(off, woff) and np.array_equal(tc, wtc)


# ---- 1. equality with the restatement
@pytest.mark.parametrize('h,w', SHAPES)
def test_boundary_and_maps_equal_the_restatement(h, w):
    st = seeded_stack(h, w)
    maps, edge = ref_maps(h, w)
    # N = 3 with 5 channels; N = 1 with 4 (the float4 pack), with 4 from a base 4 bytes off alignment, and with 1
    variants = [(dev(st), slice(0, 3), slice(0, 5)), (dev(st[:1, :, :, :4]), slice(0, 1), slice(0, 4)),
                (misaligned(st[:1, :, :, 1:5]), slice(0, 1), slice(1, 5)), (dev(st[1:2, :, :, 2:3]), slice(1, 2), slice(2, 3))]
    for d, ns, cs in variants:
        before = d.clone()
        got = distance.boundary_stack(d)
        assert got.dtype == torch.float32 and got.shape == d.shape
        assert np.array_equal(host(got), edge[ns, :, :, cs])
        for part in PARTS:
            got = distance.distance_stack(d, to=part)
            assert got.dtype == torch.int32 and tuple(got.shape) == (d.shape[0], d.shape[3], h, w)
            assert np.array_equal(host(got), maps[part][ns, cs]), part
        assert torch.equal(d, before)                                    # the input stack is never modified


@pytest.mark.parametrize('src_part,dst_part', [('boundary', 'boundary'), ('set', 'set'), ('set', 'clear')])
@pytest.mark.parametrize('h,w', SHAPES)
def test_lists_minimum_and_counts_equal_the_restatement(h, w, src_part, dst_part):
    st = seeded_stack(h, w)
    want_lists, want_min, want_overlap = ref_lists(h, w, src_part, dst_part)
    d = dev(st)
    d2, off, tc, overlap = distance._lists(d, d, PAIRS, src_part, dst_part, distance.DEFAULT_SCRATCH)
    assert lists_equal((d2, off, tc), want_lists) and np.array_equal(overlap, want_overlap)
    assert lists_equal(distance.directed_distances(d, d, PAIRS, src_part, dst_part), want_lists)
    got_min = distance.pair_minimum(d, d, PAIRS, src_part, dst_part)
    assert got_min.dtype == np.uint64 and np.array_equal(got_min, want_min)
    # one slice, and two stacks of different channel counts from a misaligned base
    a, b = misaligned(st[2:3, :, :, :4]), dev(st[2:3, :, :, 1:3])
    pairs = [(0, 0), (1, 1), (2, 0), (3, 1)]
    want = R.directed(st[2:3, :, :, :4], st[2:3, :, :, 1:3], pairs, src_part, dst_part)
    assert lists_equal(distance.directed_distances(a, b, pairs, src_part, dst_part), want)
    assert np.array_equal(distance.pair_minimum(a, b, pairs, src_part, dst_part), R.pair_min(st[2:3, :, :, :4], st[2:3, :, :, 1:3], pairs, src_part, dst_part))


def test_default_pairs_are_equal_channels():
    st = seeded_stack(33, 65)
    d = dev(st)
    assert lists_equal(distance.directed_distances(d, d), R.directed(st, st, [(c, c) for c in range(5)]))
    with pytest.raises(ValueError):
        distance.directed_distances(d, d[..., :4].contiguous())
    with pytest.raises(ValueError):
        distance.directed_distances(d, d, [(0, 5)])


# ---- 2. designed planes
def designed_planes(h=70, w=130):
    z = np.zeros((h, w), bool)
    planes = {'empty': z.copy(), 'full': ~z}
    for name, (y, x) in {'corner_tl': (0, 0), 'corner_tr': (0, w - 1), 'corner_bl': (h - 1, 0), 'corner_br': (h - 1, w - 1)}.items():
        planes[name] = z.copy()
        planes[name][y, x] = True
    ends = z.copy()                              # objects whose right edge sits at column 63 / 64 / 65 ...
    ends[5:15, 55:64] = True
    ends[25:35, 55:65] = True
    ends[45:55, 55:66] = True
    starts = z.copy()                            # ... and whose left edge does
    starts[5:15, 63:75] = True
    starts[25:35, 64:75] = True
    starts[45:55, 65:75] = True
    planes['edge_ends'], planes['edge_starts'] = ends, starts
    two = z.copy()
    two[5, 10] = two[5, 30] = True               # (5, 20) is equidistant from both
    planes['equidistant'] = two
    return planes


def test_designed_planes():
    planes = designed_planes()
    names = sorted(planes)
    st = np.stack([planes[k] for k in names], axis=-1)[None].astype(np.float32)
    d = dev(st)
    h, w = st.shape[1:3]
    ch = {k: i for i, k in enumerate(names)}
    edge = host(distance.boundary_stack(d))
    assert np.array_equal(edge, R.boundary_stack(st))
    ring = np.ones((h, w), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(edge[0, :, :, ch['full']], ring) and not edge[0, :, :, ch['empty']].any()
    maps = {p: host(distance.distance_stack(d, to=p)) for p in PARTS}
    for p in PARTS:
        assert np.array_equal(maps[p], R.distance_stack(st, p)), p
    assert (maps['set'][0, ch['empty']] == distance.DIST_NONE).all() and (maps['boundary'][0, ch['empty']] == distance.DIST_NONE).all()
    assert (maps['clear'][0, ch['full']] == distance.DIST_NONE).all() and (maps['set'][0, ch['full']] == 0).all()
    assert (maps['clear'][0, ch['empty']] == 0).all()
    yy, xx = np.mgrid[:h, :w]
    for name, (y, x) in {'corner_tl': (0, 0), 'corner_tr': (0, w - 1), 'corner_bl': (h - 1, 0), 'corner_br': (h - 1, w - 1)}.items():
        assert np.array_equal(maps['set'][0, ch[name]], (yy - y) ** 2 + (xx - x) ** 2), name      # the row search runs the whole row
    assert maps['set'][0, ch['equidistant'], 5, 20] == 100 and maps['set'][0, ch['equidistant'], 15, 20] == 200
    pairs = [(ch['edge_ends'], ch['edge_starts']), (ch['edge_starts'], ch['edge_ends']), (ch['corner_tl'], ch['corner_br']),
             (ch['full'], ch['empty']), (ch['empty'], ch['full']), (ch['equidistant'], ch['equidistant'])]
    for sp, dp in (('boundary', 'boundary'), ('set', 'set')):
        assert lists_equal(distance.directed_distances(d, d, pairs, sp, dp), R.directed(st, st, pairs, sp, dp))
        assert np.array_equal(distance.pair_minimum(d, d, pairs, sp, dp), R.pair_min(st, st, pairs, sp, dp))
    key = distance.pair_minimum(d, d, [(ch['corner_tl'], ch['corner_br'])])[0, 0]
    assert int(key) == ((h - 1) ** 2 + (w - 1) ** 2) << 32


@pytest.mark.parametrize('h,w', [(1, 4096), (4096, 1)])
def test_longest_row_and_column(h, w):
    """The only target at the far end of the longest frame the kernels take: d2 = 4095^2 at the near end, the edge of the uint16 column
    distance and far inside int32."""
    st = np.zeros((1, h, w, 1), np.float32)
    st[0, h - 1, w - 1, 0] = 1
    d = dev(st)
    got = host(distance.distance_stack(d, to='set'))[0, 0]
    want = (4095 - np.arange(4096, dtype=np.int64)) ** 2
    assert got[0, 0] == 4095 ** 2 and np.array_equal(got.reshape(-1), want)
    assert np.array_equal(host(distance.boundary_stack(d)), st)
    near = np.zeros_like(st)
    near[0, 0, 0, 0] = 1
    d2, off, tc = distance.directed_distances(dev(near), d)
    assert d2.tolist() == [4095 ** 2] and off.tolist() == [0, 1] and tc.tolist() == [[1]]
    assert int(distance.pair_minimum(dev(near), d)[0, 0]) == (4095 ** 2) << 32


# ---- 3. chunking
def test_results_do_not_depend_on_the_chunking():
    h, w = 97, 130
    st = seeded_stack(h, w)
    d = dev(st)
    lib = L.lib()
    one = int(lib.octseg_distance_scratch_bytes(1, h, w, 5, 0, 0))
    one_pair = int(lib.octseg_distance_scratch_bytes(1, h, w, 5, 5, len(PAIRS)))
    assert int(lib.octseg_distance_scratch_bytes(3, h, w, 5, 0, 0)) > 2 * one      # the default budget takes all three slices at once
    for budget in (one, 2 * one + 1, 1):
        assert torch.equal(distance.boundary_stack(d, scratch_bytes=budget), distance.boundary_stack(d))
        assert torch.equal(distance.distance_stack(d, to='boundary', scratch_bytes=budget), distance.distance_stack(d, to='boundary'))
    whole = distance._lists(d, d, PAIRS, 'boundary', 'boundary', distance.DEFAULT_SCRATCH)
    whole_min = distance.pair_minimum(d, d, PAIRS)
    for budget in (one_pair, 2 * one_pair + 1):
        got = distance._lists(d, d, PAIRS, 'boundary', 'boundary', budget)
        assert all(np.array_equal(a, b) for a, b in zip(got, whole))
        assert np.array_equal(distance.pair_minimum(d, d, PAIRS, scratch_bytes=budget), whole_min)
    assert lists_equal(whole[:3], ref_lists(h, w, 'boundary', 'boundary')[0])


# ---- 4. capacity
def test_a_short_key_buffer_raises_and_nothing_is_stored_past_it():
    """The guard of the key store is what is under test: positions at or past the capacity are dropped on the device."""
    h, w = 33, 65
    st = seeded_stack(h, w)
    d = dev(st)
    (want_d2, want_off, _), _, _ = ref_lists(h, w, 'boundary', 'boundary')
    total = int(want_off[-1])
    assert total > 100
    npairs, dims = len(PAIRS), (3, h, w, 5, 5)
    pairs_dev = torch.tensor(PAIRS, dtype=torch.int32, device='cuda')
    offsets = torch.from_numpy(want_off[:-1].copy()).cuda()
    guard = 64
    keys = torch.full((total + guard,), -7, dtype=torch.int64, device='cuda')
    distance._fill_keys(d, d, pairs_dev, npairs, 2, 2, dims, offsets, keys, total, distance.DEFAULT_SCRATCH)
    assert (keys[total:] == -7).all()
    got = torch.sort(keys[:total]).values
    assert np.array_equal(host(got & 0xffffffff), want_d2)
    assert np.array_equal(np.bincount(host(got >> 32), minlength=3 * npairs), np.diff(want_off))
    keys.fill_(-7)
    with pytest.raises(RuntimeError, match='key buffer'):
        distance._fill_keys(d, d, pairs_dev, npairs, 2, 2, dims, offsets, keys, total - 1, distance.DEFAULT_SCRATCH)
    torch.cuda.synchronize()
    assert (keys[total - 1:] == -7).all()                               # the dropped key's slot and the guard tail are untouched
    assert int((keys[:total - 1] != -7).sum()) == total - 1
    # offsets that point past the buffer altogether: every key of those segments is dropped, none is stored anywhere
    keys.fill_(-7)
    with pytest.raises(RuntimeError, match='key buffer'):
        distance._fill_keys(d, d, pairs_dev, npairs, 2, 2, dims, offsets + (1 << 40), keys, total, distance.DEFAULT_SCRATCH)
    torch.cuda.synchronize()
    assert (keys == -7).all()


# ---- 5. six slices of the pullback fixture
@functools.lru_cache(maxsize=None)
def golden():
    """Slices 27 .. 32 of the fixture: lumen everywhere, cap and lipid core on 28 .. 30, vasa vasorum on 30 .. 32."""
    st = load_fixture(FIXTURE)['stack'][27:33].astype(np.float32)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def golden_ref():
    st = golden()
    pairs = [(c, c) for c in range(4)]
    return (R.directed(st[:5], st[1:], pairs), R.directed(st[1:], st[:5], pairs), R.overlap(st[:5], st[1:], pairs),
            R.pair_min(st, st, [(2, 0)], 'set', 'set'))


def test_golden_slices_surface_metrics():
    st = golden()
    ab, ba, overlap, _ = golden_ref()
    pred, truth = dev(st[:5]), dev(st[1:])
    d2, offsets, counts = distance._surface_lists(pred, truth, [(c, c) for c in range(4)])
    assert lists_equal((d2[0], offsets[0], ab[2]), ab) and lists_equal((d2[1], offsets[1], ba[2]), ba) and np.array_equal(counts, overlap)
    got = distance.surface_metrics(pred, truth)
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert got == distance.build_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), overlap, names)
    assert list(got) == names and got['Lumen']['slice'] == [0, 1, 2, 3, 4] and None not in got['Lumen']['hd']
    assert got['Lipid core']['hd'][0] is None and got['Lipid core']['hd'][1] is not None and got['Lipid core']['dice'][4] == 1.0
    for col in got.values():
        for hd, hd95, assd in zip(col['hd'], col['hd95'], col['assd']):
            assert hd is None or (0 < assd <= hd and 0 <= hd95 <= hd)
    quarter = distance.surface_metrics(pred, truth, ratio=4)
    assert quarter['Lumen']['hd'] == [v / 4 for v in got['Lumen']['hd']] and quarter['Lumen']['dice'] == got['Lumen']['dice']


def test_golden_slices_cap_distance():
    st = golden()
    want = golden_ref()[3]
    d = dev(st)
    assert np.array_equal(distance.pair_minimum(d, d, [(2, 0)], 'set', 'set'), want)
    got = distance.cap_distance(d)
    assert got == distance.build_cap_distance(want[:, 0], 750)
    assert got['slice'] == [1, 2, 3] and got['d2'] == [617, 218, 265] and got['at'] == [(444, 283), (441, 291), (446, 293)]
    assert got['distance'][1] == pytest.approx(218 ** 0.5)
    named = distance.cap_distance(d, classes=['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum'], ratio=112)
    assert named['d2'] == got['d2'] and named['distance'] == pytest.approx([v / 112 for v in got['distance']], rel=1e-15)
    with pytest.raises(ValueError):
        distance.cap_distance(d[..., :2].contiguous())


def test_wrappers_refuse_wrong_dtype_rank_and_extents():
    for bad in (torch.zeros((1, 4, 4, 4), dtype=torch.float64, device='cuda'), torch.zeros((4, 4, 4), device='cuda'),
                torch.zeros((1, 0, 4, 4), device='cuda'), torch.zeros((1, 4, 4, 17), device='cuda'), torch.zeros((1, 1, 4097, 1), device='cuda')):
        for fn in (distance.boundary_stack, distance.distance_stack, lambda s: distance.directed_distances(s, s), distance.cap_distance):
            with pytest.raises(ValueError):
                fn(bad)
