"""File dataset and batch source -- host half of the input pipeline.

Mirror of ``OCTDataset`` / ``OCTDataModule`` (reference ``src/models/smp/dataset.py:20-158``) without Lightning, joblib and tqdm.
The reference resizes every frame and mask on the CPU inside ``__getitem__``; here ``OCTDataset`` only pairs and decodes the files
and hands out the UNDECIMATED uint8 arrays, and ``DeviceBatches`` uploads them as uint8 and lets the GPU do the rest
(``ingest.resize_image_u8`` / ``select_resize_mask``): 3 bytes per source pixel cross the bus instead of 12 per output sample.

    train = train_batches(cfg, 'train')          # re-iterable: one pass per epoch, what fit() asks for
    model, history = fit(cfg, train, train_batches(cfg, 'test'))

Augmentation stays in ``fit()`` (``use_augmentation`` -> ``octseg_augment``).  Iterating needs a GPU: there is no CPU path.
"""
import logging
import os
from glob import glob

import numpy as np
import torch
from PIL import Image

from .model import CLASS_IDS
from .parallel import shard_range


def read_image_bgr(path):
    """``cv2.imread(path)``: uint8 [H, W, 3] in BGR order; grey files come back as three equal planes, alpha is dropped."""
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def read_mask_tiff(path):
    """``tifffile.imread(path)`` where tifffile imports, Pillow's reader otherwise (a 4-channel uint8 TIFF reads back the same)."""
    try:
        import tifffile
    except ImportError:
        with Image.open(path) as im:
            return np.array(im)
    return tifffile.imread(path)


class OCTDataset:
    """dataset.py:76-158.  ``__getitem__`` -> ``(img_bgr uint8 [H, W, 3], mask uint8 [H, W, Cs])`` at the files' own size."""

    def __init__(self, data_dir, classes, input_size=512, read_mask=None):
        self.classes = list(classes)
        self.class_ids = [CLASS_IDS[cl] for cl in self.classes]
        self.input_size = int(input_size)
        self.read_mask = read_mask if read_mask is not None else read_mask_tiff
        mask_paths = sorted(glob(os.path.join(data_dir, 'mask', '*.tiff')))
        pairs = [self.verify_pairs(os.path.join(data_dir, 'img'), p, self.class_ids, self.read_mask) for p in mask_paths]
        pairs = [p for p in pairs if p is not None]
        if not pairs:
            raise ValueError('Warning: No correct data found')
        self.img_paths, self.mask_paths = zip(*pairs)

    @staticmethod
    def verify_pairs(img_dir, mask_path, class_ids, read_mask=read_mask_tiff):
        """dataset.py:132-152: the pair counts if the image exists and some selected channel holds a value above 1."""
        stem = os.path.splitext(os.path.basename(mask_path))[0]
        img_path = os.path.join(img_dir, f'{stem}.png')
        if not os.path.exists(img_path):
            logging.warning(f'Image: {img_path} does not exist')
            return None
        mask = np.asarray(read_mask(mask_path))
        if mask.ndim == 2:
            mask = mask[:, :, None]
        for class_id in class_ids:
            if np.any(mask[:, :, class_id - 1] > 1):
                return img_path, mask_path
        return None

    def __len__(self):
        return len(self.img_paths)

    def __getitem__(self, idx):
        img = read_image_bgr(self.img_paths[idx])
        mask = np.asarray(self.read_mask(self.mask_paths[idx]))
        if mask.ndim == 2:
            mask = mask[:, :, None]
        if mask.dtype != np.uint8:      # only `!= 0` of a mask sample is ever used (dataset.py:117): one byte per sample is enough
            mask = (mask != 0).astype(np.uint8)
        return img, np.ascontiguousarray(mask)


def group_by_shape(shapes):
    """Positions of a batch grouped by source shape, groups in order of first appearance: [(shape, [positions])]."""
    groups = {}
    for pos, shape in enumerate(shapes):
        groups.setdefault(tuple(shape), []).append(pos)
    return list(groups.items())


class DeviceBatches:
    """Re-iterable batch source over an ``OCTDataset`` (``OCTDataModule``'s two DataLoaders, dataset.py:59-73): every pass is one epoch
    and yields ``(img [B,3,S,S] float32 0..255 BGR, mask [B,C,S,S] float32 0/1)`` CUDA tensors.

    The frames of a batch are grouped by source size; each group goes through one pinned uint8 staging buffer, one ``non_blocking``
    host-to-device copy and one launch per kernel that writes the group's frames into the batch tensors; all of it on a side stream that
    the caller's current stream waits on (an event) before the batch is handed out.  The order inside a batch is the epoch's order with
    the frames of one source size together.

    Data parallel: pass the same ``seed`` on every rank; rank r takes ``parallel.shard_range`` of each epoch's permutation.  With
    ``drop_last`` every rank yields the same number of (full) batches, which the gradient all-reduce of ``fit()`` needs.

    ``side_stream=False`` enqueues copy and kernels on the caller's stream instead (a measurement aid: tools/bench_ingest.py)."""

    def __init__(self, dataset, batch_size, shuffle=False, seed=None, device='cuda', rank=0, world=1, drop_last=False, side_stream=True):
        if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError(f'bad batch_size / rank / world: {batch_size}, {rank}, {world}')
        if shuffle and seed is None:
            if world > 1:
                raise ValueError('shuffle under data parallel needs the same seed on every rank')
            seed = int(np.random.SeedSequence().entropy % (2 ** 32))
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, int(batch_size), bool(shuffle), seed
        self.device, self.rank, self.world, self.drop_last = device, int(rank), int(world), bool(drop_last)
        self.side_stream = bool(side_stream)
        self.epoch = 0
        self._side = None
        self._pinned = {}     # 'img' / 'mask' -> (pinned uint8 buffer, event of the last copy that read it)

    # ---- bookkeeping: plain numpy, no device
    def epoch_order(self, epoch):
        """Dataset indices of epoch ``epoch`` (0-based) before sharding: a permutation drawn from (seed, epoch), or 0..n-1."""
        n = len(self.dataset)
        if not self.shuffle:
            return np.arange(n)
        return np.random.default_rng([int(self.seed), int(epoch)]).permutation(n)

    def shard(self, epoch):
        order = self.epoch_order(epoch)
        lo, hi = shard_range(len(order), self.rank, self.world)
        return order[lo:hi]

    def num_batches(self):
        n = len(self.dataset)
        if self.drop_last:
            return (n // self.world) // self.batch_size      # the smallest shard's full batches, on every rank
        lo, hi = shard_range(n, self.rank, self.world)
        return -(-(hi - lo) // self.batch_size)

    __len__ = num_batches

    def batch_indices(self, epoch):
        """This rank's batches of epoch ``epoch``: a list of index arrays."""
        idx = self.shard(epoch)
        nb = self.num_batches()
        return [idx[i * self.batch_size:(i + 1) * self.batch_size] for i in range(nb)]

    # ---- device half
    def _staging(self, kind, nbytes):
        buf, ev = self._pinned.get(kind, (None, None))
        if ev is not None:
            ev.synchronize()          # the previous batch's copy out of this buffer
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True)
        return buf

    def upload(self, samples):
        """[(img_bgr uint8 [H,W,3], mask uint8 [H,W,Cs])] -> the batch's two CUDA tensors (see the class docstring)."""
        from . import ingest
        if not torch.cuda.is_available():
            raise RuntimeError('DeviceBatches needs a GPU: the input pipeline has no CPU path')
        dev = torch.device(self.device)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        consumer = torch.cuda.current_stream(dev)
        if self._side is None and self.side_stream:
            self._side = torch.cuda.Stream(device=dev)
        side = self._side if self.side_stream else consumer
        S, ids, B = self.dataset.input_size, self.dataset.class_ids, len(samples)
        groups = group_by_shape([(s[0].shape, s[1].shape) for s in samples])
        nbytes = {'img': sum(samples[p][0].nbytes for _, ps in groups for p in ps),
                  'mask': sum(samples[p][1].nbytes for _, ps in groups for p in ps)}
        with torch.cuda.stream(side):
            img = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
            mask = torch.empty((B, len(ids), S, S), dtype=torch.float32, device=dev)
            stage = {k: self._staging(k, n) for k, n in nbytes.items()}
            off, at = {'img': 0, 'mask': 0}, 0
            for (ishape, mshape), ps in groups:
                if ishape[:2] != mshape[:2]:
                    # the reference resizes both to input_size independently; so does this path, but a pair of different sizes is a data error
                    logging.warning(f'image {ishape} and mask {mshape} differ in size')
                dev_u8 = {}
                for k, shape, j in (('img', ishape, 0), ('mask', mshape, 1)):
                    n1 = int(np.prod(shape))
                    host = stage[k][off[k]:off[k] + n1 * len(ps)]
                    view = host.numpy().reshape((len(ps),) + tuple(shape))
                    for g, p in enumerate(ps):
                        view[g] = samples[p][j]
                    dev_u8[k] = host.to(dev, non_blocking=True).view((len(ps),) + tuple(shape))
                    off[k] += n1 * len(ps)
                ingest.resize_image_u8(dev_u8['img'], S, out=img[at:at + len(ps)])
                ingest.select_resize_mask(dev_u8['mask'], ids, S, out=mask[at:at + len(ps)])
                at += len(ps)
            done = side.record_event()
            self._pinned = {k: (stage[k], done) for k in stage}
        if side is not consumer:
            consumer.wait_event(done)
            img.record_stream(consumer)      # allocated on the side stream, used on the caller's: the allocator must not recycle them early
            mask.record_stream(consumer)
        return img, mask

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        for idx in self.batch_indices(epoch):
            yield self.upload([self.dataset[int(i)] for i in idx])


def train_batches(cfg, split='train', device='cuda'):
    """``OCTDataModule.setup('fit')`` + ``train_dataloader`` / ``val_dataloader`` (dataset.py:40-73) from train.yaml's keys:
    ``<data_dir>/<split>``, ``classes``, ``input_size``, ``batch_size``; the 'train' split is shuffled.  Under torchrun every rank gets its
    shard (``cfg['seed']``, default 0, must agree across ranks) and full batches only."""
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    ds = OCTDataset(os.path.join(cfg['data_dir'], split), cfg['classes'], cfg['input_size'])
    seed = cfg.get('seed', 0 if world > 1 else None)
    return DeviceBatches(ds, cfg['batch_size'], shuffle=(split == 'train'), seed=seed, device=device, rank=rank, world=world,
                         drop_last=(world > 1 and split == 'train'))
