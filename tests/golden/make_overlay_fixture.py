"""A window of one of the reference's published demo runs, as a fixture for the rendering tests (tests/test_postprocess.py,
tests/test_gpu_postprocess.py).

The reference ships three finished predictions: data/demo/input/<name>.png -> data/demo/output/<name>_{mask,overlay}.png, written by its
save_results (src/data/utils.py:195-235).  This script copies DATA only: of frame 006_1_100, rows 600:920 and columns 360:680 of
  frame    Image.open(input).resize((1000, 1000)).convert('RGB')    what data_processing hands to save_results
  mask     the authors' colour mask                                (128,128,128) + class colours; anti-aliased at the class borders, because
                                                                   the masks of that run were not binary there
  overlay  the authors' overlay
into tests/golden/demo_overlay_crop.npz.  No program text of the reference is read or copied.

    python tests/golden/make_overlay_fixture.py <path of the reference checkout>
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = '006_1_100'
ROWS, COLS = (600, 920), (360, 680)


def main(ref_root):
    demo = os.path.join(ref_root, 'data', 'demo')
    frame = np.asarray(Image.open(os.path.join(demo, 'input', f'{NAME}.png')).resize((1000, 1000)).convert('RGB'))
    mask = np.asarray(Image.open(os.path.join(demo, 'output', f'{NAME}_mask.png')).convert('RGB'))
    overlay = np.asarray(Image.open(os.path.join(demo, 'output', f'{NAME}_overlay.png')).convert('RGB'))
    assert frame.shape == mask.shape == overlay.shape == (1000, 1000, 3), (frame.shape, mask.shape, overlay.shape)
    win = (slice(*ROWS), slice(*COLS))
    out = os.path.join(HERE, 'demo_overlay_crop.npz')
    np.savez_compressed(out, frame=frame[win], mask=mask[win], overlay=overlay[win], rows=np.array(ROWS), cols=np.array(COLS))
    print(f'wrote {out}: {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
