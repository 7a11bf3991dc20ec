"""The operating curves without a GPU: the cases' margin rule and the agreement of the f32 and the float64 bin rule on every pixel of them (the
condition under which tests/test_gpu_curves.py compares whole histograms by equality), the host curves against scikit-learn and against direct
counts, the tie rules, the ABI's declaration and refusals, the wrappers' and the serving switch's checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import curves_cases as CC
import curves_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import curves

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('case', CC.CASES, ids=CC.IDS)
def test_cases_keep_the_margin_and_both_rules_bin_them_identically(case):
    z, t = CC.inputs(case)
    assert z.dtype == np.float32 and t.dtype == np.float32 and z.shape == case.shape == t.shape
    if case.kind.startswith('sat-'):
        assert (np.abs(z) == 30).all() and (z > 0).any() and (z < 0).any()
        for bins in (R.bins64, R.bins32):       # the clamp decides: bin 0 / bin 255 on either arithmetic
            assert np.array_equal(bins(z), np.where(z > 0, 255, 0))
    else:
        assert CC.margin_ok(z).all()
    if case.kind == 'zeros':
        assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
        assert (R.bins64(z) == 127).all()                                   # p = 0.5 exactly: not above the threshold 128 / 256
    assert np.array_equal(R.bins32(z), R.bins64(z))
    ref = CC.reference(case)
    assert np.array_equal(R.histogram(z, t, R.bins32), ref)
    assert ref.shape == case.shape[:2] + (2, 256) and (ref.sum(axis=(2, 3)) == case.shape[2] * case.shape[3]).all()
    assert np.array_equal(ref[:, :, 1].sum(axis=2), (t != 0).sum(axis=(2, 3)))


def test_sanitize_replaces_what_the_margin_rule_names():
    edge = np.float32(np.log(64 / 192))                                     # p * 256 = 64 up to rounding
    z = np.array([edge, 0.0, -0.0, 20.0, -20.0, 1.0, CC.MID], dtype=np.float32)
    assert CC.margin_ok(z).tolist() == [False, True, True, False, False, True, True]
    s = CC.sanitize(z)
    assert s.tolist() == [CC.MID, 0.0, 0.0, CC.MID, CC.MID, 1.0, CC.MID] and np.signbit(s[2]) and CC.margin_ok(s).all()
    assert R.bins64(CC.MID) == 37 and abs(R.sigmoid64(CC.MID) * 256 - 37.5) < 1e-4
    rng = np.random.default_rng(0)
    raw = (rng.standard_normal(11766) * 3.0).astype(np.float32)
    share = 1.0 - CC.margin_ok(raw).mean()
    print(f'share of a N(0, 3^2) draw inside the margin: {share:.4%}')
    assert 0 < share < 0.01


@pytest.mark.parametrize('case', [c for c in CC.CASES if c.kind == 'drawn' and np.prod(c.shape) > 1], ids=lambda c: c.id)
def test_k128_row_equals_direct_counts_of_z_above_zero(case):
    z, t = CC.inputs(case)
    cur = curves.operating_curves(CC.reference(case))                       # pooled over the frames
    want = R.counts_at(z, t, 0.0).sum(axis=0)
    got = np.stack([cur[k][:, 128] for k in ('tp', 'fp', 'fn', 'tn')], axis=-1)
    assert np.array_equal(got, want)
    hw = case.shape[0] * case.shape[2] * case.shape[3]
    for k in ('tp', 'fp', 'fn', 'tn'):
        assert cur[k].dtype == np.int64 and cur[k].shape == (case.shape[1], 257)
    assert (cur['tp'] + cur['fp'] + cur['fn'] + cur['tn'] == hw).all()
    assert (cur['fn'][:, 0] == 0).all() and (cur['tn'][:, 0] == 0).all()     # k = 0 sets everything
    assert (cur['tp'][:, 256] == 0).all() and (cur['fp'][:, 256] == 0).all()  # k = 256 sets nothing
    # every other threshold too: bin >= k is p > k / 256, i.e. z > logit(k / 256), which the margin keeps clear of every z
    for k in (1, 37, 64, 200, 255):
        cut = np.log((k / 256) / (1 - k / 256))
        assert np.array_equal(np.stack([cur[m][:, k] for m in ('tp', 'fp', 'fn', 'tn')], axis=-1), R.counts_at(z, t, cut).sum(axis=0)), k


def test_metrics_at_128_are_the_epoch_csvs():
    from oct_segmentation_amd.metrics import _metrics_from_numpy
    case = CC.CASES[0]
    z, t = CC.inputs(case)
    stats = R.counts_at(z, t, 0.0)                                          # [N, C, 4], what the Dice kernel emits
    per_frame = curves._curves(np.array(CC.reference(case)))
    want = _metrics_from_numpy(stats, np.float32(0))
    for k in ('dice', 'iou', 'precision', 'recall'):
        assert per_frame[k].dtype == np.float64 and np.array_equal(per_frame[k][..., 128], want[k].astype(np.float64)), k
    empty = np.zeros((1, 2, 256), dtype=np.int64)
    empty[0, 0, 3] = 10                                                     # no positive pixel, nothing set at 128: 0 / 0 -> 1e-7
    cur = curves.operating_curves(empty)
    assert cur['iou'][0, 128] == np.float64(np.float32(1e-7)) and np.isnan(cur['auc'][0]) and np.isnan(cur['ap'][0])


@pytest.mark.parametrize('case', [CC.CASES[0], CC.CASES[2], CC.CASES[3]], ids=lambda c: c.id)
def test_auc_and_ap_equal_sklearn_on_the_bin_indices(case):
    from sklearn.metrics import average_precision_score, roc_auc_score
    z, t = CC.inputs(case)
    cur = curves.operating_curves(CC.reference(case))
    scores, labels = R.bins64(z), (t != 0)
    for c in range(case.shape[1]):
        y, s = labels[:, c].ravel(), scores[:, c].ravel()
        auc, ap = roc_auc_score(y, s), average_precision_score(y, s)
        print(f'{case.id} class {c}: auc {cur["auc"][c]:.15f} (sklearn {auc:.15f}), ap {cur["ap"][c]:.15f} (sklearn {ap:.15f})')
        assert abs(cur['auc'][c] - auc) <= 1e-12 * auc
        assert abs(cur['ap'][c] - ap) <= 1e-12 * ap


def test_reliability_table_and_ece_use_bin_midpoints():
    h = np.zeros((1, 2, 256), dtype=np.int64)
    h[0, 0, 25], h[0, 1, 25] = 30, 10                                       # bin 25: 40 pixels, a quarter positive, midpoint 25.5 / 256
    h[0, 1, 255] = 60                                                       # bin 255: 60 pixels, all positive, midpoint 255.5 / 256
    cur = curves.operating_curves(h)
    assert cur['bin_count'][0, 25] == 40 and cur['bin_positive'][0, 25] == 0.25 and cur['bin_mid'][25] == 25.5 / 256
    assert np.isnan(cur['bin_positive'][0, 0]) and cur['bin_count'][0].sum() == 100
    want = 0.4 * abs(0.25 - 25.5 / 256) + 0.6 * abs(1.0 - 255.5 / 256)
    assert abs(cur['ece'][0] - want) < 1e-15
    both = curves.operating_curves(np.stack([h, h]))                         # per frame [N, C, 2, 256]: summed first
    assert np.array_equal(both['tp'], 2 * cur['tp']) and abs(both['ece'][0] - want) < 1e-15
    assert np.array_equal(curves.operating_curves(torch.from_numpy(h).int())['tp'], cur['tp'])
    with pytest.raises(ValueError, match='hist'):
        curves.operating_curves(np.zeros((2, 128), dtype=np.int64))
    with pytest.raises(ValueError, match='hist'):
        curves.operating_curves(np.zeros((1, 2, 256), dtype=np.float32))


def test_best_thresholds_tie_rules():
    def hist(pos_bins, neg_bins):
        h = np.zeros((1, 2, 256), dtype=np.int64)
        for j in pos_bins:
            h[0, 1, j] += 10
        for j in neg_bins:
            h[0, 0, j] += 10
        return h
    # positives in bin 200, negatives in bin 50: every k in 51..200 separates them perfectly -> the k nearest 128 is 128 itself
    b = curves.best_thresholds(hist([200], [50]))
    assert b['k'].tolist() == [128] and b['threshold'].tolist() == [0.5] and b['best'][0] == 1.0 and b['at_half'][0] == 1.0
    # the perfect range 141..200 lies above 128: its end nearest 128
    b = curves.best_thresholds(hist([200], [140]))
    assert b['k'].tolist() == [141] and b['best'][0] == 1.0 and b['at_half'][0] < 1.0
    # ... below 128: 31..100 -> 100
    b = curves.best_thresholds(hist([100], [30]))
    assert b['k'].tolist() == [100] and b['best'][0] == 1.0 and b['at_half'][0] == 0.0          # nothing set at 128, ten positives missed
    # two perfect ranges at the same distance from 128, 119..120 and 136..137 -> |k - 128| = 8 twice: the smaller k
    h = hist([137, 120], [])                                                 # positives only: dice(k) = 2 tp / (2 tp + fn)
    h[0, 0, 135] = 10
    h[0, 0, 118] = 10
    b = curves.best_thresholds(h)
    cur = curves.operating_curves(h)
    top = np.flatnonzero(cur['dice'][0, 1:256] == cur['dice'][0, 1:256].max()) + 1
    assert b['k'][0] == min(top, key=lambda k: (abs(k - 128), k))
    # a symmetric tie, made by hand from the values: _pick sees only the curve
    v = np.zeros(257)
    v[[120, 136]] = 1.0
    assert curves._pick(v) == 120
    v[[0, 256]] = 2.0                                                        # the end points are not candidates
    assert curves._pick(v) == 120
    v[130] = 1.0
    assert curves._pick(v) == 130
    assert curves.best_thresholds(hist([200], [50]), metric='iou')['k'].tolist() == [128]
    with pytest.raises(ValueError, match='metric'):
        curves.best_thresholds(hist([200], [50]), metric='f2')


def test_curve_report_is_json_and_holds_both_thresholds():
    case = CC.CASES[0]
    h = CC.reference(case)
    names, classes = ['b', 'a'], ['Lumen', 'Lipid core', 'Fibrous cap']
    rep = curves.curve_report(h, names, classes)
    assert json.loads(json.dumps(rep)) == rep and rep['bins'] == 256 and rep['frames'] == 2 and len(rep['thresholds']) == 257
    cur, best, frames = curves.operating_curves(h), curves.best_thresholds(h), curves._curves(np.array(h))
    for c, cls in enumerate(classes):
        e = rep['classes'][cls]
        assert e['best_k'] == best['k'][c] and e['best_threshold'] == best['k'][c] / 256
        assert e['dice_at_half'] == cur['dice'][c, 128] and e['dice_at_best'] == cur['dice'][c, e['best_k']] >= e['dice_at_half']
        assert e['auc'] == cur['auc'][c] and e['ap'] == cur['ap'][c] and e['ece'] == cur['ece'][c]
        assert e['curves']['tp'] == cur['tp'][c].tolist() and e['curves']['dice'] == cur['dice'][c].tolist()
        assert e['pixels'] == 2 * 37 * 53 and e['positive_pixels'] == cur['tp'][c, 0]
        assert list(e['slices']) == names
        for i, name in enumerate(names):
            assert e['slices'][name] == {'dice_at_half': frames['dice'][i, c, 128], 'dice_at_best': frames['dice'][i, c, e['best_k']]}
        assert sum(e['reliability']['count']) == e['pixels'] and len(e['reliability']['midpoint']) == 256
    with pytest.raises(ValueError, match='names'):
        curves.curve_report(h, ['a'], classes)
    with pytest.raises(ValueError, match='class names'):
        curves.curve_report(h, names, classes[:2])
    with pytest.raises(ValueError, match='per-frame'):
        curves.curve_report(np.array(h).sum(axis=0), names, classes)


def test_library_exports_the_symbol_with_the_declared_signature():
    lib = L.lib()
    _P = C.c_void_p
    assert hasattr(lib, 'octseg_logit_histogram')
    assert L.SYMBOLS['octseg_logit_histogram'] == (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P, _P])
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    assert 'int octseg_logit_histogram(const float* logits, const float* target, int N, int classes, int H, int W,' in header
    assert '#define OCTSEG_CURVE_BINS 256' in header and curves.BINS == 256 and R.BINS == 256
    assert ' *   octseg_logit_histogram ' in header                                       # the table at the top
    assert 'clamp((int)ceilf(p * 256.0f) - 1, 0, 255)' in header                          # the bin rule the reference is written from


def test_abi_refusals_need_no_gpu():
    lib = L.lib()
    one = 8      # any non-null pointer value: every refusal below happens before any HIP call

    def call(logits=one, target=one, N=2, classes=3, H=8, W=8, hist=one):
        return lib.octseg_logit_histogram(logits, target, N, classes, H, W, hist, None)

    err = lambda: lib.octseg_last_error().decode()                                       # noqa: E731
    for name in ('logits', 'target', 'hist'):
        assert call(**{name: None}) == -5 and 'null' in err(), name
    for kw in ({'N': 0}, {'classes': 0}, {'H': 0}, {'W': -1}, {'N': -3}):
        assert call(**kw) == -1 and '<= 0' in err(), kw
    assert call(H=65536, W=32768) == -1 and '2^31' in err()                                # H * W = 2^31
    assert call(H=46341, W=46341) == -1 and '2^31' in err()                                # the product overflows an int
    assert call(N=65536, classes=1) == -1 and '65536 planes' in err()
    assert call(N=256, classes=256) == -1 and '65536 planes' in err()
    assert call(N=65536, classes=65536) == -1                                              # N * classes overflows an int: refused all the same
    assert call(N=0, logits=None) == -5                                                    # the null is named first


def test_wrappers_refuse_host_tensors_wrong_dtypes_and_shapes():
    z = torch.zeros((1, 1, 4, 4))
    with pytest.raises(ValueError, match='CUDA'):
        curves.logit_histograms(z, z)
    with pytest.raises(ValueError, match='float32'):
        curves.logit_histograms(z.double(), z)
    with pytest.raises(ValueError, match='logits'):
        curves.logit_histograms(z.numpy(), z)
    with pytest.raises(ValueError, match='float32 tensor'):
        curves.apply_thresholds(z.double(), [0], [0.4])
    with pytest.raises(ValueError, match='float32 tensor'):
        curves.apply_thresholds(z[0], [0], [0.4])


def test_apply_thresholds_shifts_in_place_and_refuses_bad_values():
    z = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2) - 10
    before = z.clone()
    out = curves.apply_thresholds(z, [2, 0], [0.25, 0.8])
    assert out is z
    assert torch.equal(z[:, 1], before[:, 1])
    assert torch.equal(z[:, 2], before[:, 2] - float(np.float32(np.log(0.25 / 0.75))))
    assert torch.equal(z[:, 0], before[:, 0] - float(np.float32(np.log(0.8 / 0.2))))
    assert curves.threshold_shift(0.5) == 0 and curves.threshold_shift(0.25).dtype == np.float32
    half = before.clone()
    half[0, 0, 0, 0] = -0.0
    want = half.clone()
    curves.apply_thresholds(half, [0, 1, 2], [0.5, 0.5, 0.5])
    assert torch.equal(half.view(torch.int32), want.view(torch.int32))                    # t = 0.5 changes no bit, not even -0.0's sign
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'\(0, 1\)'):
            curves.apply_thresholds(z, [0], [bad])
    with pytest.raises(ValueError, match='channel 3'):
        curves.apply_thresholds(z, [3], [0.4])
    with pytest.raises(ValueError, match='twice'):
        curves.apply_thresholds(z, [1, 1], [0.4, 0.6])
    with pytest.raises(ValueError, match='one entry'):
        curves.apply_thresholds(z, [1], [0.4, 0.6])
    kept = z.clone()
    with pytest.raises(ValueError):
        curves.apply_thresholds(z, [0, 1], [0.4, 2.0])                                    # refused as a whole: channel 0 is not shifted either
    assert torch.equal(z, kept)


def test_predict_reads_the_thresholds_key(tmp_path):
    from oct_segmentation_amd.config import load_config
    from oct_segmentation_amd.predict import _threshold_key
    cfg = load_config('predict')
    assert 'thresholds' not in cfg and _threshold_key(cfg) is None                        # configs/predict.yaml stays the reference's
    cfg = load_config('predict', ['thresholds={"Lumen": 0.4, "Fibrous cap": 0.75}'])
    assert _threshold_key(cfg) == {'Lumen': 0.4, 'Fibrous cap': 0.75}
    rep = curves.curve_report(CC.reference(CC.CASES[0]), ['a', 'b'], ['Lumen', 'Lipid core', 'Fibrous cap'])
    path = str(tmp_path / 'curves.json')
    with open(path, 'w') as f:
        json.dump(rep, f)
    got = _threshold_key(load_config('predict', [f'thresholds={path}']))
    assert got == {k: rep['classes'][k]['best_threshold'] for k in ('Lumen', 'Lipid core', 'Fibrous cap')}
    for bad, match in (('{"Lumen": 0.4, "Media": 0.5}', 'unknown class'), ('{"Lumen": 1.0}', r'\(0, 1\)'), ('{"Lumen": 0}', r'\(0, 1\)'),
                       ('{"Lumen": "high"}', 'number'), ('{"Lumen": true}', 'number'), ('{}', 'non-empty'), ('[0.4]', 'non-empty'), ('0.4', 'dict')):
        with pytest.raises(ValueError, match=match):
            _threshold_key(load_config('predict', [f'thresholds={bad}']))
    with pytest.raises(ValueError, match='unknown class'):                                # segment_stack checks before it loads anything
        from oct_segmentation_amd.predict import segment_stack
        segment_stack([], [8, 8], ['Lumen'], str(tmp_path), thresholds={'Media': 0.4})
    with pytest.raises(ValueError, match='unknown class'):
        from oct_segmentation_amd.vote import segment_stack_voted
        segment_stack_voted(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [8, 8], ['Lumen'], str(tmp_path), thresholds={'Media': 0.4})


def test_tool_arguments():
    cfg = curves._config(['model_dir=m', 'data_dir=d'])
    assert cfg == {'model_dir': 'm', 'data_dir': 'd', 'batch_size': 8, 'compute_dtype': 'bf16', 'save_dir': None, 'device': 'auto'}
    assert curves._config(['model_dir=m', 'data_dir=d', 'batch_size=2', 'compute_dtype=fp32', 'save_dir=s'])['batch_size'] == 2
    for bad in (['data_dir=d'], ['model_dir=m'], ['model_dir=m', 'data_dir=d', 'epochs=3'], ['model_dir=m', 'data_dir=d', 'batch_size=0'],
                ['model_dir=m', 'data_dir=d', 'compute_dtype=fp8'], ['model_dir']):
        with pytest.raises(ValueError):
            curves._config(bad)
