"""Planes of the reference's demo pullback for the clean-up tests (tests/test_cleanup.py, tests/test_gpu_cleanup.py).

The reference's app ships one finished pullback: data/app/demo/mask/*.tiff, 186 masks of 750 x 750 x 4 with values 0 / 255 (channel =
CLASS_ID - 1).  The script reads those files as data and picks
  * the two Vasa vasorum planes with four 8-connected components (files 129 and 159, counted from 1); one carries two components of equal
    area (144 / 144), the tie of the keep-3 rule;
  * every plane that scipy.ndimage.binary_fill_holes changes (a scan finds four: two Lumen, one Lipid core, one Vasa vasorum).

Output: tests/golden/cleanup_demo_masks.npz
  packed, shape      np.packbits of the boolean [P, 750, 750] planes, and that shape
  slices, channels   the 1-based file number and the channel of every plane
  ncomp, holes       recorded for the tests: 8-connected components per plane, and the pixels binary_fill_holes adds

    python tests/golden/make_cleanup_fixture.py <path of the reference checkout>
"""
import os
import sys
from glob import glob

import numpy as np
from PIL import Image
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
VASA = 3
FOUR_COMPONENT_SLICES = (129, 159)


def main(ref_root):
    files = sorted(glob(os.path.join(os.path.abspath(ref_root), 'data', 'app', 'demo', 'mask', '*.tiff')))
    assert len(files) == 186, len(files)
    full = np.ones((3, 3), np.int32)
    picked = []
    for i, f in enumerate(files):
        m = np.asarray(Image.open(f)) != 0
        assert m.shape == (750, 750, 4), m.shape
        for c in range(4):
            plane = m[:, :, c]
            if not plane.any():
                continue
            n = ndimage.label(plane, structure=full)[1]
            holes = int(ndimage.binary_fill_holes(plane).sum() - plane.sum())
            if holes or (c == VASA and i + 1 in FOUR_COMPONENT_SLICES):
                if c == VASA and i + 1 in FOUR_COMPONENT_SLICES:
                    assert n == 4, (i + 1, n)
                picked.append((i + 1, c, n, holes, plane))
    planes = np.stack([p[4] for p in picked])
    out = os.path.join(HERE, 'cleanup_demo_masks.npz')
    np.savez_compressed(out, packed=np.packbits(planes), shape=np.array(planes.shape), slices=np.array([p[0] for p in picked], np.int32),
                        channels=np.array([p[1] for p in picked], np.int32), ncomp=np.array([p[2] for p in picked], np.int32),
                        holes=np.array([p[3] for p in picked], np.int32))
    print(f'wrote {out}: {os.path.getsize(out)} bytes; (slice, channel, components, hole pixels) = {[p[:4] for p in picked]}')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
