"""An excerpt of the reference's demo pullback with what the REFERENCE's own code measures on it, as a fixture for the analysis tests
(tests/test_analysis.py, tests/test_gpu_analysis.py).

The reference's app ships one finished pullback: data/app/demo/mask/*.tiff, 186 masks of 750 x 750 x 4 with values 0 / 255.  Its
src/app/tools/analysis.py is loaded with importlib straight from the reference checkout and executed unmodified; nothing of its text is
copied.  The module imports packages that are not installed, so they are stubbed in sys.modules for the import:
  * cv2       -- findContours returns no contours (calculate_thickness_contour then returns 0: that value is NOT recorded), plus the two flags
                 the call names;
  * gradio    -- Progress / Slider / Plot / Markdown / Checkboxgroup / JSON as inert callables (the UI half of get_analysis' return value);
  * pydicom   -- dcmread returns an object whose pixel_array is a [48, 750, 750] array (get_analysis takes only its shape: ratio = 112);
  * tifffile  -- imread decodes the mask with PIL;
  * src.app.tools.img_viewer, src.app.tools.plotly_analytics -- get_object_map returns its argument, so the first return value of
                 get_analysis is its `data` dict; the plot helpers return None;
  * src.data.utils -- the class ids (src/data/utils.py:16-45).
Input: the slices with 0-based index 84..131 of the sorted demo masks -- Lumen throughout; Fibrous cap and Lipid core with a run that ends,
isolated groups of 1-3 slices and gaps; Vasa vasorum as single-slice objects.  get_analysis runs in `demo` mode from a temporary directory
that holds those 48 files as data/app/demo/mask.

Output: tests/golden/pullback_demo_excerpt.npz
  packed, shape      np.packbits of the boolean [48, 750, 750, 4] stack, and that shape
  names              the 48 file stems
  objects_json       {'ratio', 'objects': {class: {'slice', 'area', 'object_id', 'img_name'}}, 'images'} from get_analysis
  thick_*            for every present (slice, class): what calculate_object_thickness returns -- slice, channel, median, min, max, and
                     all_measurements concatenated (thick_all) with their lengths (thick_len)

    python tests/golden/make_pullback_fixture.py <path of the reference checkout>
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types
from glob import glob

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, LAST = 84, 131
CLASS_IDS = {'Lumen': 1, 'Fibrous cap': 2, 'Lipid core': 3, 'Vasa vasorum': 4}


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference_analysis(ref_root, n_slices, size):
    inert = lambda *a, **k: None                                                           # noqa: E731
    _module('cv2', findContours=lambda *a, **k: ([], None), RETR_EXTERNAL=0, CHAIN_APPROX_SIMPLE=2)
    _module('gradio', Progress=inert, Slider=inert, Plot=inert, Markdown=inert, Checkboxgroup=inert, JSON=inert)
    _module('pydicom', dcmread=lambda f: types.SimpleNamespace(pixel_array=np.broadcast_to(np.uint8(0), (n_slices, size, size))))
    _module('tifffile', imread=lambda p: np.asarray(Image.open(p)))
    for pkg in ('src', 'src.app', 'src.app.tools', 'src.data'):
        _module(pkg).__path__ = []
    _module('src.app.tools.img_viewer', get_img_show=inert)
    _module('src.app.tools.plotly_analytics', get_object_map=lambda data: data, get_plot_area=inert, get_trace_area=inert)
    _module('src.data.utils', CLASS_IDS=CLASS_IDS, CLASS_IDS_REVERSED={v: k for k, v in CLASS_IDS.items()})
    spec = importlib.util.spec_from_file_location('reference_app_analysis', os.path.join(ref_root, 'src', 'app', 'tools', 'analysis.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref_root = os.path.abspath(ref_root)
    files = sorted(glob(os.path.join(ref_root, 'data', 'app', 'demo', 'mask', '*.tiff')))[FIRST:LAST + 1]
    assert len(files) == LAST - FIRST + 1, len(files)
    stack = np.stack([np.asarray(Image.open(f)) for f in files])
    assert stack.shape == (len(files), 750, 750, 4) and stack.dtype == np.uint8 and set(np.unique(stack)) <= {0, 255}, (stack.shape, stack.dtype)
    names = [os.path.basename(f).split('.')[0] for f in files]
    ref = load_reference_analysis(ref_root, len(files), stack.shape[1])

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'data', 'app', 'demo', 'mask'))
        for f in files:
            shutil.copy(f, os.path.join(tmp, 'data', 'app', 'demo', 'mask'))
        os.chdir(tmp)
        try:
            data = ref.get_analysis('pullback.dcm', 'demo')[0]
        finally:
            os.chdir(cwd)
    objects = {cl: {k: [v if isinstance(v, str) else (int(v) if k != 'area' else float(v)) for v in obj[k]]
                    for k in ('slice', 'area', 'object_id', 'img_name')} for cl, obj in data['objects'].items()}
    recorded = {'ratio': int(data['ratio']), 'objects': objects, 'images': list(data['images'])}
    assert recorded['images'] == names

    rows = []
    for cl, obj in objects.items():
        ch = CLASS_IDS[cl] - 1
        for idx in obj['slice']:
            t = ref.calculate_object_thickness(stack[idx, :, :, ch])
            rows.append((idx, ch, float(t['median']), int(t['min']), int(t['max']), [int(v) for v in t['all_measurements']]))
    rows.sort()                                                                            # by (slice, channel)
    all_meas = [v for r in rows for v in r[5]]
    out = os.path.join(HERE, 'pullback_demo_excerpt.npz')
    np.savez_compressed(out, packed=np.packbits(stack != 0), shape=np.array(stack.shape), names=np.array(names),
                        objects_json=np.array(json.dumps(recorded)),
                        thick_slice=np.array([r[0] for r in rows], np.int32), thick_channel=np.array([r[1] for r in rows], np.int32),
                        thick_median=np.array([r[2] for r in rows], np.float64), thick_min=np.array([r[3] for r in rows], np.int32),
                        thick_max=np.array([r[4] for r in rows], np.int32), thick_len=np.array([len(r[5]) for r in rows], np.int32),
                        thick_all=np.array(all_meas, np.int16))
    print(f'wrote {out}: {os.path.getsize(out)} bytes, {len(rows)} present (slice, class) masks, '
          f'{ {cl: len(o["slice"]) for cl, o in objects.items()} }')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
