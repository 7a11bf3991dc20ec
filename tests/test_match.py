"""Lesion matching without a GPU: the ABI's declarations and refusals, the wrappers' argument checks, the restatement the GPU tests hold the kernels
to (tests/match_ref.py) proved against sklearn's contingency matrix on every case the GPU test uses and on the demo excerpt, build_match on
hand-written tables, and the command line with the device part stubbed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lesions_ref as LR
import match_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import match

HERE = os.path.dirname(os.path.abspath(__file__))


def test_library_exports_the_new_symbols_with_the_declared_signatures():
    lib = L.lib()
    _P = C.c_void_p
    want = {'octseg_match_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
            'octseg_volume_match': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P, _P, _P, _P])}
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert L.SYMBOLS[name] == (res, args)
        assert f'{name}(' in header
    assert ' *   octseg_volume_match / octseg_match_scratch_bytes\n' in header                    # the table at the top
    assert ('int octseg_volume_match(const float* pred, const float* truth, int N, int H, int W, int channels, int across, void* scratch, '
            'size_t scratch_bytes,\n                        int* nles, int* top, int* overlap, int* frames, void* stream);') in header
    assert 'size_t octseg_match_scratch_bytes(int channels, int N, int H, int W);' in header
    assert match.RANKS == 33 and match.TOPL == 32 and match.ACROSS == {'overlap': 0, 'full': 1}


def test_scratch_formula_and_that_the_lesions_formula_did_not_move():
    lib = L.lib()
    sb = lib.octseg_match_scratch_bytes
    al = lambda v: (v + 255) // 256 * 256                                                          # noqa: E731
    # parent of either side + vox + zmax (4 B per voxel each), the shared lesion list, the counter and the threshold, 32 ranked roots per side,
    # nles and top side by side, two sets of bits; every part rounded up to 256 bytes
    for c, n, h, w in ((2, 3, 5, 70), (1, 1, 1, 1), (16, 2, 9, 129), (4, 186, 704, 704)):
        v, w64 = c * n * h * w, (w + 63) // 64
        want = (4 * al(4 * v) + al(4 * c * n * ((h + 1) // 2) * ((w + 1) // 2)) + 2 * al(4 * c) + 2 * al(4 * c * 32) + al(4 * c * 2)
                + al(4 * c * 2 * 32 * 8) + 2 * al(8 * c * n * h * w64))
        assert sb(c, n, h, w) == want, (c, n, h, w)
        assert sb(c, n, h, w) < 2 * lib.octseg_lesions_scratch_bytes(c, n, h, w) or n * h * w < 4096      # below two labellings' worth
    assert lib.octseg_lesions_scratch_bytes(2, 3, 5, 70) == 3 * al(2 * 3 * 350 * 4) + al(2 * 3 * 3 * 35 * 4) + 2 * al(2 * 4) + al(2 * 32 * 4) + \
        2 * al(2 * 3 * 5 * 2 * 8)
    assert sb(0, 2, 4, 4) == 0 and sb(17, 2, 4, 4) == 0 and sb(1, 0, 4, 4) == 0 and sb(1, 2, 0, 4) == 0 and sb(1, 2, 4, -1) == 0
    assert sb(1, 1 << 11, 1 << 10, 1 << 10) == 0 and sb(1, 2, 1 << 15, 1 << 15) == 0                 # N * H * W = 2^31
    assert sb(1, 1, 2 ** 31 - 1, 1) == 0 and sb(1, 1, 2 ** 31 - 2, 1) > 0                             # refused from 2^31 - 1 on


def test_abi_refusals_need_no_gpu_and_name_the_argument():
    lib = L.lib()
    one = 8      # any non-null, 8-byte aligned pointer value: every refusal below happens before any HIP call
    big = 1 << 50
    buf = C.create_string_buffer(64)                                                              # real memory for the outputs: stays zero
    out = C.addressof(buf)

    def call(pred=one, truth=one, N=2, H=4, W=4, ch=4, across=0, scratch=one, nbytes=big, nles=out, top=out, overlap=out, frames=out):
        return lib.octseg_volume_match(pred, truth, N, H, W, ch, across, scratch, nbytes, nles, top, overlap, frames, None)

    for kw, code, word in (({'pred': None}, -5, b'pred'), ({'truth': None}, -5, b'truth'), ({'scratch': None}, -5, b'scratch'),
                           ({'nles': None}, -5, b'nles'), ({'overlap': None}, -5, b'overlap'), ({'scratch': 12}, -5, b'aligned'),
                           ({'nbytes': lib.octseg_match_scratch_bytes(4, 2, 4, 4) - 1}, -5, b'octseg_match_scratch_bytes'),
                           ({'nbytes': 0}, -5, b'scratch'), ({'across': 2}, -5, b'across'), ({'across': -1}, -5, b'across'),
                           ({'N': 0}, -1, b'empty'), ({'H': 0}, -1, b'empty'), ({'W': -1}, -1, b'empty'), ({'ch': 0}, -1, b'channels'),
                           ({'ch': 17}, -1, b'channels'), ({'N': 2, 'H': 1 << 15, 'W': 1 << 15}, -1, b'2^31'),
                           ({'N': 1, 'H': 2 ** 31 - 1, 'W': 1}, -1, b'2^31')):
        assert call(**kw) == code, kw
        msg = lib.octseg_last_error()
        assert word in msg and b'volume_match' in msg, (kw, msg)
    assert not any(buf.raw)


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    host = torch.zeros((2, 4, 4, 4))
    for fn in (match.match_volumes, match.match_report):
        for bad in (host, np.zeros((2, 4, 4, 4), np.float32), torch.zeros((2, 4, 4, 4), dtype=torch.float64), torch.zeros((4, 4, 4))):
            with pytest.raises(ValueError, match='float32 CUDA tensor'):
                fn(bad, bad)
        for bad in ('6', 'OVERLAP', 26, None):
            with pytest.raises(ValueError, match='across'):
                fn(host, host, across=bad)
    with pytest.raises(ValueError, match='unknown build_match keywords'):
        match.match_report(host, host, smooth=3)


# ---- the restatement against sklearn
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_restatement_equals_sklearn_contingency_on_every_gpu_case(name):
    pred, truth = R.case(name)
    for across in ('overlap', 'full'):
        nles, top, overlap, frames = R.case_tables(name, across)
        for c in range(pred.shape[3]):
            p, t = pred[..., c] != 0, truth[..., c] != 0
            assert np.array_equal(overlap[c], R.contingency_by_rank(p, t, across)), (across, c)
            assert int(overlap[c].sum()) == int((p & t).sum()) == int(frames[c, :, 0].sum())
            assert (overlap[c, :32].sum(axis=1) <= top[c, 0, :, 0]).all() and (overlap[c, :, :32].sum(axis=0) <= top[c, 1, :, 0]).all()
            for side, vol in enumerate((p, t)):
                n1, t1, _ = LR.table(vol, across)
                assert nles[c, side] == n1 and np.array_equal(top[c, side], t1)
                assert np.array_equal(frames[c, :, 1 + side], vol.reshape(vol.shape[0], -1).sum(axis=1))


def test_restatement_on_designed_cases_by_hand():
    nles, top, overlap, frames = R.case_tables('same', 'overlap')
    for c in range(2):
        assert nles[c, 0] == nles[c, 1] <= 32 and np.array_equal(top[c, 0], top[c, 1])
        assert np.array_equal(overlap[c], np.diag(np.concatenate([top[c, 0, :, 0], [0]])))           # the diagonal equals the voxels
    assert not R.case_tables('disjoint', 'full')[2].any() and not R.case_tables('empty', 'overlap')[2].any()
    nles, top, overlap, frames = R.case_tables('inner_runs', 'overlap')
    assert nles.tolist() == [[2, 2], [2, 2]]
    assert overlap[0, :2, :2].tolist() == [[18, 0], [0, 18]] and overlap[1, :2, :2].tolist() == [[18, 0], [0, 18]]
    nles, top, overlap, frames = R.case_tables('cover_two', 'overlap')
    assert nles.tolist() == [[1, 2], [2, 1]] and (overlap[0, 0, :2] > 0).all() and (overlap[1, :2, 0] > 0).all()
    nles, top, overlap, frames = R.case_tables('thirty_four', 'overlap')
    assert nles.tolist() == [[34, 34]] and overlap[0].sum() == 34 * 4
    assert overlap[0, 32, 32] == 8 and overlap[0, 32, :32].sum() == 0 and overlap[0, :32, 32].sum() == 0 and (np.diag(overlap[0])[:32] == 4).all()
    nles, top, overlap, frames = R.case_tables('late_join', 'overlap')
    assert nles.tolist() == [[2, 1], [1, 2]] and (overlap[0, :2, 0] > 0).all() and (overlap[1, 0, :2] > 0).all()
    assert R.case_tables('late_join', 'overlap')[1][0, 1, 0, 1] < 9 * 65                              # the joined lesion's first voxel is in slice 0


def test_restatement_on_the_golden_excerpt_against_a_shifted_copy():
    """A 12-slice, 512 x 512 window of the demo excerpt (where all four classes show) against itself moved by (4, 6) pixels: the whole excerpt
    would spend a minute in scipy's labelling, and the window holds the same kind of lesions."""
    stack, names, _ = LR.golden_stack()
    stack, names = stack[10:22, 120:632, 120:632], names[10:22]
    shifted = np.zeros_like(stack)
    shifted[:, 4:, 6:] = stack[:, :-4, :-6]
    nles, top, overlap, frames = R.tables(shifted, stack, 'overlap')
    assert (nles > 0).all() and (nles <= 32).all()
    for c in range(4):
        assert np.array_equal(overlap[c], R.contingency_by_rank(shifted[..., c], stack[..., c], 'overlap')), c
        assert int(overlap[c].sum()) == int((shifted[..., c] & stack[..., c]).sum()) > 0
        assert np.array_equal(top[c, 1], LR.table(stack[..., c], 'overlap')[1])
    rep = match.build_match(nles, top, overlap, frames, 512, 512, image_names=names)
    R.assert_report_equals_scores(rep, R.scores(nles, top, overlap, frames), ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum'])
    assert rep['Lumen']['tp'] == 1 and rep['Lumen']['pq'] == rep['Lumen']['sq'] > 0.9 and not rep['Lumen']['truncated']


# ---- build_match
def hand_tables():
    """Three classes, N = 4.  a: pred 0 = truth 0 exactly at 2 I == union (no match at 0.5), pred 1 matches truth 1, truth 2 is split over pred
    2 and 3, pred 4 merges truth 3 and 4.  b: nothing on either side.  c: 40 against 33 lesions, overlap in the rest row and column."""
    nles = np.array([[5, 5], [0, 0], [40, 33]], np.int32)
    top = np.zeros((3, 2, 32, 8), np.int32)
    overlap = np.zeros((3, 33, 33), np.int32)
    frames = np.zeros((3, 4, 3), np.int32)
    vp, vt = [30, 20, 8, 7, 30], [30, 22, 18, 16, 15]
    for i in range(5):
        top[0, 0, i] = [vp[i], i, 0, 1 + i % 2, 0, 1, 0, 1]
        top[0, 1, i] = [vt[i], i, i % 2, 2, 0, 1, 0, 1]
    overlap[0, 0, 0] = 20            # union 40: 2 I == union
    overlap[0, 1, 1] = 19            # union 23
    overlap[0, 2, 2] = 8
    overlap[0, 3, 2] = 6
    overlap[0, 4, 3] = 16
    overlap[0, 4, 4] = 5
    frames[0] = [[40, 50, 50], [43, 55, 51], [0, 0, 0], [0, 0, 3]]
    top[2, :, :, 0] = 2
    top[2, :, :, 3] = 1
    overlap[2, 0, 0] = 2
    overlap[2, 32, 1] = 1
    overlap[2, 32, 32] = 3
    overlap[2, 5, 32] = 2
    frames[2] = [[8, 80, 66], [0, 0, 0], [0, 1, 0], [0, 0, 0]]
    return nles, top, overlap, frames


def test_build_match_on_hand_written_tables():
    nles, top, overlap, frames = hand_tables()
    names = [f's{i}' for i in range(4)]
    rep = match.build_match(nles, top, overlap, frames, 10, 20, image_names=names, classes=['a', 'b', 'c'])
    assert list(rep) == ['a', 'b', 'c'] and json.loads(json.dumps(rep)) == rep                    # plain numbers: the JSON round trip
    R.assert_report_equals_scores(rep, R.scores(nles, top, overlap, frames), ['a', 'b', 'c'])
    a = rep['a']
    assert [(p['pred'], p['truth']) for p in a['pairs']] == [(0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (4, 4)]
    assert a['pairs'][0]['iou'] == 0.5 and a['pairs'][0]['dice'] == 2 / 3 and a['matches'] == [[1, 1], [4, 3]]      # the exact tie does not match
    assert a['pairs'][1] == {'pred': 1, 'truth': 1, 'intersection': 19, 'iou': 19 / 23, 'dice': 38 / 42, 'length_pred': 3, 'length_truth': 2,
                             'start_offset': -1, 'end_offset': 0}
    assert (a['tp'], a['fp'], a['fn']) == (2, 3, 3) and a['sensitivity'] == 0.4 and a['precision'] == 0.4 and a['f1'] == 0.4
    assert a['sq'] == (19 / 23 + 16 / 30) / 2 and a['rq'] == 2 / 5 and a['pq'] == a['sq'] * a['rq']
    assert a['split'] == 1 and a['merged'] == 1 and a['truncated'] is False and a['unranked_overlap'] == {'pred_rest': 0, 'truth_rest': 0}
    assert a['voxel_dice'] == 2 * 83 / (105 + 104)
    assert a['frames'] == {'min_pixels': 1, 'tp': 2, 'fp': 0, 'fn': 1, 'tn': 1, 'sensitivity': 2 / 3, 'specificity': 1.0,
                           'dice': [0.8, 86 / 106, None, 0.0], 'images': names}
    b = rep['b']
    assert b['n_pred'] == b['n_truth'] == 0 and b['pairs'] == [] and (b['tp'], b['fp'], b['fn']) == (0, 0, 0)
    for key in ('sensitivity', 'precision', 'f1', 'sq', 'rq', 'pq', 'voxel_dice'):
        assert b[key] is None, key                                                               # empty denominators
    assert b['frames']['sensitivity'] is None and b['frames']['specificity'] == 1.0 and b['frames']['dice'] == [None] * 4
    c = rep['c']
    assert c['truncated'] is True and c['n_pred'] == 40 and c['n_truth'] == 33 and c['unranked_overlap'] == {'pred_rest': 4, 'truth_rest': 5}
    assert (c['tp'], c['fp'], c['fn']) == (1, 31, 31) and c['pairs'][0]['iou'] == 1.0
    assert rep['a']['frames']['tn'] == 1 and match.build_match(nles, top, overlap, frames, 10, 20, min_pixels=2)['Lumen']['frames']['tn'] == 1
    assert match.build_match(nles, top, overlap, frames, 10, 20, min_pixels=4)['Lumen']['frames']['fn'] == 0
    # a stricter threshold, decided in float64
    strict = match.build_match(nles, top, overlap, frames, 10, 20, iou=0.6)
    assert strict['Lumen']['matches'] == [[1, 1]] and strict['Lumen']['iou_threshold'] == 0.6
    R.assert_report_equals_scores(strict, R.scores(nles, top, overlap, frames, iou=0.6), ['Lumen', 'Fibrous cap', 'Lipid core'])
    # the overlap criterion
    for mo in (1, 7, 15):
        ovr = match.build_match(nles, top, overlap, frames, 10, 20, classes=['a', 'b', 'c'], criterion='overlap', min_overlap=mo)
        R.assert_report_equals_scores(ovr, R.scores(nles, top, overlap, frames, criterion='overlap', min_overlap=mo), ['a', 'b', 'c'])
        assert json.loads(json.dumps(ovr)) == ovr and 'tp' not in ovr['a']
    ovr = match.build_match(nles, top, overlap, frames, 10, 20, classes=['a', 'b', 'c'], criterion='overlap')
    assert (ovr['a']['detected'], ovr['a']['missed'], ovr['a']['false_positives']) == (5, 0, 0) and ovr['a']['sensitivity'] == 1.0
    assert (ovr['c']['detected'], ovr['c']['missed'], ovr['c']['false_positives']) == (2, 30, 30)     # truth 1 through the rest row
    assert ovr['b']['sensitivity'] is None and ovr['b']['precision'] is None
    seven = match.build_match(nles, top, overlap, frames, 10, 20, classes=['a', 'b', 'c'], criterion='overlap', min_overlap=7)['a']
    assert (seven['detected'], seven['false_positives']) == (4, 1)                                # truth 4 by 5, pred 3 by 6 only
    for bad in (dict(image_names=names[:-1]), dict(classes=['a', 'b']), dict(classes=['a', 'a', 'b']), dict(criterion='dice'), dict(iou=0.49),
                dict(iou=1.0), dict(min_overlap=0), dict(min_pixels=0)):
        with pytest.raises(ValueError):
            match.build_match(nles, top, overlap, frames, 10, 20, **bad)
    for bad in ((nles[:, :1], top, overlap, frames), (nles, top[:, :, :8], overlap, frames), (nles, top, overlap[:, :32], frames),
                (nles, top, overlap, frames[:2])):
        with pytest.raises(ValueError):
            match.build_match(*bad, 10, 20)


# ---- the command line
def test_main_on_two_tiff_directories(tmp_path, monkeypatch, capsys):
    from PIL import Image
    pred_dir, truth_dir, save_dir = tmp_path / 'pred', tmp_path / 'truth', tmp_path / 'out'
    pred_dir.mkdir()
    truth_dir.mkdir()
    pred, truth = R.case('seeded_2x9x64')
    for folder, st in ((pred_dir, pred), (truth_dir, truth)):
        for i in range(2):
            Image.fromarray((st[i] * 255).astype(np.uint8)).save(str(folder / f's{i}.tiff'))
    Image.fromarray(np.zeros((9, 64, 4), np.uint8)).save(str(pred_dir / 'unpaired.tiff'))
    seen = []

    def tables(p, t, across):                                  # what the GPU would return, from the restatement
        seen.append(across)
        assert np.array_equal(np.asarray(p) != 0, pred != 0) and np.array_equal(np.asarray(t) != 0, truth != 0)
        return R.tables(p, t, across)
    monkeypatch.setattr(match, '_host_tables', tables)
    report = match.main([str(pred_dir), str(truth_dir), str(save_dir), 'across=full', 'iou=0.75'])
    path = save_dir / 'lesion_match.json'
    assert capsys.readouterr().out.strip() == str(path)
    saved = json.load(open(path))
    assert saved == json.loads(json.dumps(report)) and seen == ['full']
    classes = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert saved['images'] == ['s0.tiff', 's1.tiff'] and saved['classes'] == classes and saved['across'] == 'full'
    want = R.tables(pred, truth, 'full')
    R.assert_report_equals_scores(saved['match'], json.loads(json.dumps(R.scores(*want, iou=0.75))), classes)
    assert saved['match']['Lumen']['iou_threshold'] == 0.75 and saved['match']['Lumen']['frames']['images'] == ['s0.tiff', 's1.tiff']
    match.main([str(pred_dir), str(truth_dir)])                                                   # defaults: beside the predictions
    assert seen == ['full', 'overlap'] and os.path.exists(pred_dir / 'lesion_match.json')
    for bad in ([str(pred_dir)], [str(pred_dir), str(truth_dir), 'across=6'], [str(pred_dir), str(truth_dir), 'iou=0.3'],
                [str(pred_dir), str(truth_dir), 'iou=x'], [str(pred_dir), str(truth_dir), str(save_dir), 'extra']):
        with pytest.raises(SystemExit):
            match.main(bad)
