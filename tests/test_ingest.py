"""Host half of the input pipeline (oct_segmentation_amd/dataset.py, ingest.py): file pairing and decoding against the reference's
OCTDataset (src/models/smp/dataset.py:76-158), DeviceBatches' epoch / shard / batch bookkeeping, argument checks.  No GPU needed."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oct_segmentation_amd import ingest
from oct_segmentation_amd.dataset import DeviceBatches, OCTDataset, group_by_shape
from oct_segmentation_amd.model import CLASS_IDS


def _write_pair(root, stem, img, mask, with_image=True):
    os.makedirs(os.path.join(root, 'img'), exist_ok=True)
    os.makedirs(os.path.join(root, 'mask'), exist_ok=True)
    if with_image:
        Image.fromarray(img).save(os.path.join(root, 'img', f'{stem}.png'))
    Image.fromarray(mask, mode='RGBA').save(os.path.join(root, 'mask', f'{stem}.tiff'))


def _mask(rng, h, w, live_channels, high=256):
    m = np.zeros((h, w, 4), np.uint8)
    for c in live_channels:
        m[:, :, c] = rng.integers(0, high, (h, w), dtype=np.uint8)
        m[0, 0, c] = max(2, high - 1) if high > 2 else 1
    return m


def test_dataset_pairs_filters_and_decodes(tmp_path):
    rng = np.random.default_rng(0)
    root = str(tmp_path)
    imgs = {s: rng.integers(0, 256, (20, 30, 3), dtype=np.uint8) for s in ('a', 'b', 'c', 'd', 'e')}
    masks = {'a': _mask(rng, 20, 30, [0, 1]),            # Lumen + Fibrous cap live
             'b': _mask(rng, 20, 30, [2]),               # only Lipid core (channel 2) live: dropped for ['Fibrous cap', 'Lumen']
             'c': _mask(rng, 20, 30, [1], high=2),       # selected channel holds 0 / 1 only: dropped (verify_pairs wants a value > 1)
             'd': _mask(rng, 20, 30, [1]),               # no image: dropped
             'e': _mask(rng, 20, 30, [0, 1, 2, 3])}
    for s in imgs:
        _write_pair(root, s, imgs[s], masks[s], with_image=(s != 'd'))
    grey = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    os.remove(os.path.join(root, 'img', 'e.png'))
    Image.fromarray(grey).save(os.path.join(root, 'img', 'e.png'))
    classes = ['Fibrous cap', 'Lumen']
    ds = OCTDataset(root, classes, input_size=64)
    assert len(ds) == 2
    assert [os.path.basename(p) for p in ds.img_paths] == ['a.png', 'e.png']
    assert [os.path.basename(p) for p in ds.mask_paths] == ['a.tiff', 'e.tiff']
    assert ds.class_ids == [CLASS_IDS['Fibrous cap'], CLASS_IDS['Lumen']] == [2, 1]       # the order of `classes`, not sorted
    img, mask = ds[0]
    assert img.dtype == np.uint8 and mask.dtype == np.uint8
    assert np.array_equal(img, imgs['a'][:, :, ::-1])          # the PNG holds RGB, cv2.imread hands out BGR
    assert np.array_equal(mask, masks['a'])                   # undecimated, every source channel
    img, mask = ds[1]
    assert img.shape == (20, 30, 3) and all(np.array_equal(img[:, :, c], grey) for c in range(3))   # grey -> three equal planes
    # a class whose channel is live only in 'b' and 'e'
    assert [os.path.basename(p) for p in OCTDataset(root, ['Lipid core'], 64).mask_paths] == ['b.tiff', 'e.tiff']
    # the reader can be replaced; wider masks are reduced to 0 / 1 bytes
    ds16 = OCTDataset(root, classes, 64, read_mask=lambda p: np.array(Image.open(p)).astype(np.uint16) * 256)
    m16 = ds16[0][1]
    assert m16.dtype == np.uint8 and np.array_equal(m16, (masks['a'] != 0).astype(np.uint8))


def test_dataset_without_valid_pairs_raises(tmp_path):
    rng = np.random.default_rng(1)
    _write_pair(str(tmp_path), 'x', rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), _mask(rng, 8, 8, [0], high=2))
    with pytest.raises(ValueError, match='Warning: No correct data found'):
        OCTDataset(str(tmp_path), ['Lumen'], 64)
    with pytest.raises(ValueError, match='Warning: No correct data found'):
        OCTDataset(os.path.join(str(tmp_path), 'missing'), ['Lumen'], 64)


class _FakeDataset:
    input_size, class_ids = 64, [1]

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_device_batches_bookkeeping():
    ds = _FakeDataset(23)
    a = DeviceBatches(ds, 4, shuffle=True, seed=7)
    b = DeviceBatches(ds, 4, shuffle=True, seed=7)
    for epoch in (0, 1, 5):
        assert np.array_equal(a.epoch_order(epoch), b.epoch_order(epoch))
        assert sorted(a.epoch_order(epoch)) == list(range(23))
    assert not np.array_equal(a.epoch_order(0), a.epoch_order(1))
    assert not np.array_equal(a.epoch_order(0), DeviceBatches(ds, 4, shuffle=True, seed=8).epoch_order(0))
    assert np.array_equal(DeviceBatches(ds, 4).epoch_order(3), np.arange(23))
    # batches: every index once, short last batch kept / dropped
    bi = a.batch_indices(0)
    assert [len(x) for x in bi] == [4, 4, 4, 4, 4, 3] and len(a) == 6
    assert np.array_equal(np.concatenate(bi), a.epoch_order(0))
    d = DeviceBatches(ds, 4, shuffle=True, seed=7, drop_last=True)
    assert [len(x) for x in d.batch_indices(0)] == [4] * 5 and len(d) == 5
    # two ranks: disjoint shards that cover the epoch; with drop_last the same number of full batches on both
    for epoch in (0, 2):
        r = [DeviceBatches(ds, 4, shuffle=True, seed=7, rank=k, world=2) for k in range(2)]
        s0, s1 = r[0].shard(epoch), r[1].shard(epoch)
        assert not set(s0) & set(s1) and sorted(np.concatenate([s0, s1])) == list(range(23))
        assert np.array_equal(np.concatenate([s0, s1]), a.epoch_order(epoch))
        assert np.array_equal(np.concatenate(r[0].batch_indices(epoch)), s0)
    rd = [DeviceBatches(ds, 4, shuffle=True, seed=7, rank=k, world=2, drop_last=True) for k in range(2)]
    assert [len(x) for x in rd[0].batch_indices(0)] == [len(x) for x in rd[1].batch_indices(0)] == [4, 4]
    with pytest.raises(ValueError, match='same seed'):
        DeviceBatches(ds, 4, shuffle=True, rank=0, world=2)
    with pytest.raises(ValueError):
        DeviceBatches(ds, 0)
    # frames of one source size travel together, groups in order of first appearance
    shapes = [(1000, 1000, 3), (1024, 1024, 3), (1000, 1000, 3), (750, 750, 3), (1024, 1024, 3)]
    assert group_by_shape(shapes) == [((1000, 1000, 3), [0, 2]), ((1024, 1024, 3), [1, 4]), ((750, 750, 3), [3])]


def test_device_batches_has_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)

    class One(_FakeDataset):
        def __getitem__(self, i):
            return np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 4), np.uint8)
    with pytest.raises(RuntimeError, match='GPU'):
        next(iter(DeviceBatches(One(2), 2)))


def test_ingest_rejects_wrong_input():
    with pytest.raises(ValueError, match='uint8 CUDA'):
        ingest.resize_image_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match='uint8 CUDA'):
        ingest.select_resize_mask(torch.zeros((1, 8, 8, 4), dtype=torch.uint8), [1], 4)
    with pytest.raises(ValueError, match='uint8 CUDA'):
        ingest.resize_image_u8(np.zeros((1, 8, 8, 3), np.uint8), 4)


def test_ingest_tables_are_the_pinned_host_tables():
    """The [4, dst] layout the kernel reads is predict.cv2_linear_coeffs stacked; taps stay inside the source."""
    from oct_segmentation_amd.predict import cv2_linear_coeffs
    for src, dst in ((1000, 704), (1024, 512), (9, 1), (1, 7), (30, 23)):
        for horizontal in (True, False):
            t = ingest.linear_table(src, dst, horizontal)
            assert t.dtype == np.int32 and t.shape == (4, dst)
            for row, ref in zip(t, cv2_linear_coeffs(src, dst, horizontal=horizontal)):
                assert np.array_equal(row, ref)
            assert t[:2].min() >= 0 and t[:2].max() <= src - 1 and (np.diff(t[0]) >= 0).all() and (np.diff(t[1]) >= 0).all()
            assert (t[2:].sum(0) == 2048).all() and t[2:].min() >= 0
