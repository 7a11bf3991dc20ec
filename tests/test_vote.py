"""The voted serving epilogue without a GPU: the view algebra and the reference the GPU tests hold the kernel to (tests/vote_ref.py), the condition
under which those tests may compare EVERY pixel, find_members on directory trees, the ABI's declaration and refusals, the wrappers' checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import vote_cases as VC
import vote_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import vote

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_eight_views_form_a_group_and_unview_inverts_view():
    x = np.arange(2 * 3 * 5 * 5, dtype=np.float32).reshape(2, 3, 5, 5)
    views = [R.view(x, v) for v in range(8)]
    for v in range(8):
        assert np.array_equal(R.unview(views[v], v), x)
        assert sum(np.array_equal(views[v], views[w]) for w in range(8)) == 1            # eight different views
    table = [[R.compose(v, w) for w in range(8)] for v in range(8)]
    for v in range(8):
        assert sorted(table[v]) == list(range(8)) and sorted(row[v] for row in table) == list(range(8))     # a Latin square: closed, with inverses
        assert table[0][v] == v and table[v][0] == v
    assert table[4][1] != table[1][4]                                                    # D4 is not abelian
    assert table[4][4] == 0 and table[3][3] == 0 and R.compose(R.compose(5, 5), R.compose(5, 5)) == 0     # a quarter turn has order 4
    rect = np.arange(12, dtype=np.float32).reshape(3, 4)
    for v in range(4):
        assert R.view(rect, v).shape == (3, 4) and np.array_equal(R.unview(R.view(rect, v), v), rect)
    assert np.array_equal(R.view(rect, 1), rect[:, ::-1]) and np.array_equal(R.view(rect, 2), rect[::-1]) and R.view(rect, 4).shape == (4, 3)
    assert np.array_equal(R.view(rect, 7), rect.T[::-1, ::-1])                           # transpose first, then rows, then columns
    assert vote.VIEW_SETS == {'none': (0,), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def test_one_member_soft_is_the_plain_threshold():
    rng = np.random.default_rng(0)
    z = VC.draw_logits(rng, (2, 2, 6, 9))
    for ch in (0, 1):
        ref = R.vote([z], [ch], [0], (6, 9))
        assert np.array_equal(ref['mask'], (z[:, ch] > 0).astype(np.int64)) and not ref['dissent'].any()
        assert np.array_equal(ref['stats'][:, 0], (z[:, ch] > 0).sum(axis=(1, 2))) and not ref['stats'][:, 1:].any()
        maj = R.vote([z], [ch], [0], (6, 9), mode=1)
        assert np.array_equal(maj['mask'], ref['mask'])


def test_a_majority_tie_is_not_set():
    up, down = np.full((1, 1, 2, 2), 5.0, np.float32), np.full((1, 1, 2, 2), -0.5, np.float32)
    tie = R.vote([up, down], [0, 0], [0, 0], (2, 2), mode=1)
    assert not tie['mask'].any() and (tie['votes'] == 1).all() and (tie['dissent'] == 1).all()
    assert np.array_equal(tie['stats'], [[0, 4, 0, 4]])
    soft = R.vote([up, down], [0, 0], [0, 0], (2, 2), mode=0)                            # the confident member carries the soft vote
    assert soft['mask'].all() and (soft['dissent'] == 1).all() and np.array_equal(soft['stats'], [[4, 4, 4, 4]])
    three = R.vote([up, down, down], [0, 0, 0], [0, 0, 0], (2, 2), mode=1)
    assert not three['mask'].any() and (three['dissent'] == 1).all()


@pytest.mark.parametrize('case', VC.CASES, ids=VC.IDS)
def test_reference_properties_and_the_near_tie_condition(case):
    """Dissent off ties, the stats as sums of the maps, and: for every soft case the share of pixels with |pbar64 - 0.5| <= (M + 4) 2^-23 is exactly
    0.  Those pixels are the only ones a GPU comparison could leave out; with none of them the GPU tests compare every pixel."""
    ref = VC.reference(case)
    M = len(case.views)
    votes, mask, dissent = ref['votes'], ref['mask'].astype(bool), ref['dissent']
    assert votes.shape == (case.N, case.oh, case.ow) and votes.min() >= 0 and votes.max() <= M
    if case.mode == 1:
        assert np.array_equal(mask, 2 * votes > M)
        assert np.array_equal(dissent, np.minimum(votes, M - votes))                     # ties included: a tie is not set, so dissent = votes = M / 2
        assert (M % 2 == 1) or case.H * case.W < 4 or (2 * votes == M).any()             # even M: the case does contain ties
    else:
        off = 2 * votes != M
        agree = mask == (2 * votes > M)
        assert np.array_equal(dissent[off & agree], np.minimum(votes, M - votes)[off & agree])
        assert (np.abs(ref['pbar'] - 0.5) <= VC.prob_bound(M)).sum() == 0
    disputed = (votes > 0) & (votes < M)
    want = np.stack([mask.sum(axis=(1, 2)), disputed.sum(axis=(1, 2)), (disputed & mask).sum(axis=(1, 2)), dissent.sum(axis=(1, 2))], axis=1)
    assert np.array_equal(ref['stats'], want)
    assert (dissent == np.where(mask, M - votes, votes)).all() and (dissent[~disputed] == 0).all()


def _member(d, input_size=64, classes=('Lumen',)):
    os.makedirs(d)
    with open(os.path.join(d, 'config.json'), 'w') as f:
        json.dump({'model_name': 'm', 'architecture': 'unet', 'encoder': 'resnet18', 'input_size': input_size, 'classes': list(classes)}, f)
    open(os.path.join(d, 'weights.ckpt'), 'wb').close()


def test_find_members_orders_folds_by_number_and_falls_back(tmp_path):
    root = str(tmp_path)
    for k in (10, 2, 1):
        _member(os.path.join(root, 'LM', f'fold_{k}'))
    os.makedirs(os.path.join(root, 'LM', 'fold_3'))                                      # holds neither file: not a member
    os.makedirs(os.path.join(root, 'LM', 'fold_x'))
    assert vote.find_members(root, 'Lumen') == [os.path.join(root, 'LM', f'fold_{k}') for k in (1, 2, 10)]
    _member(os.path.join(root, 'FC_LC'), classes=('Lipid core', 'Fibrous cap'))          # today's single directory
    for name in ('Lipid core', 'Fibrous cap'):
        assert vote.find_members(root, name) == [os.path.join(root, 'FC_LC')]
    assert vote.find_members(root, 'Vasa vasorum') == [os.path.join(root, 'VV')]         # nothing there: load_model reports it
    _member(os.path.join(root, 'VV', 'fold_1'), input_size=64, classes=('Vasa vasorum',))
    _member(os.path.join(root, 'VV', 'fold_2'), input_size=96, classes=('Vasa vasorum',))
    with pytest.raises(ValueError, match='fold_2'):
        vote.find_members(root, 'Vasa vasorum')
    root2 = os.path.join(root, 'other')
    _member(os.path.join(root2, 'FC_LC', 'fold_1'), classes=('Lipid core', 'Fibrous cap'))
    _member(os.path.join(root2, 'FC_LC', 'fold_2'), classes=('Lipid core',))
    with pytest.raises(ValueError, match='differ'):
        vote.find_members(root2, 'Fibrous cap')


def test_library_exports_the_symbol_with_the_declared_signature():
    lib = L.lib()
    _P = C.c_void_p
    assert hasattr(lib, 'octseg_vote_assemble')
    assert L.SYMBOLS['octseg_vote_assemble'] == (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 4 + [_P] * 6)
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    assert 'int octseg_vote_assemble(const float* const* logits, const int* classes, const int* ch, const int* view, int M,' in header
    assert '#define OCTSEG_VOTE_MAX_MEMBERS 64' in header and vote.MAX_MEMBERS == 64
    assert ' *   octseg_vote_assemble ' in header                                         # the table at the top
    assert vote.MODES == {'soft': 0, 'majority': 1}


def test_abi_refusals_need_no_gpu_and_name_the_member():
    lib = L.lib()
    one = 8      # any non-null pointer value: every refusal below happens before any HIP call

    def call(M=3, ptrs=None, classes=(1, 2, 1), ch=(0, 1, 0), view=(0, 3, 5), N=2, H=8, W=8, mode=0, out=one, oh=8, ow=8, oc=4, out_ch=1,
             null=None):
        ptrs = [one] * len(classes) if ptrs is None else ptrs
        arrays = {'logits': (C.c_void_p * len(ptrs))(*ptrs), 'classes': (C.c_int * len(classes))(*classes), 'ch': (C.c_int * len(ch))(*ch),
                  'view': (C.c_int * len(view))(*view)}
        if null:
            arrays[null] = None
        return lib.octseg_vote_assemble(arrays['logits'], arrays['classes'], arrays['ch'], arrays['view'], M, N, H, W, mode, out, oh, ow, oc,
                                        out_ch, None, None, None, None, None, None)

    err = lambda: lib.octseg_last_error().decode()                                       # noqa: E731
    for name in ('logits', 'classes', 'ch', 'view'):
        assert call(null=name) == -5, name
    assert call(out=None) == -5
    assert call(ptrs=[one, one, None]) == -5 and 'member 2' in err()
    assert call(mode=2) == -5 and call(mode=-1) == -5 and 'mode' in err()
    assert call(M=0) == -1 and call(M=-1) == -1 and call(M=65) == -1 and '65' in err()
    for kw in ({'N': 0}, {'H': 0}, {'W': -1}, {'oh': 0}, {'ow': 0}, {'oc': 0}):
        assert call(**kw) == -1, kw
    assert call(out_ch=4) == -1 and call(out_ch=-1) == -1 and 'out_ch' in err()
    assert call(ch=(0, 2, 0)) == -1 and 'member 1' in err()
    assert call(ch=(-1, 1, 0)) == -1 and 'member 0' in err()
    assert call(classes=(1, 2, 0)) == -1 and 'member 2' in err()
    assert call(view=(0, 8, 5)) == -1 and 'member 1' in err()
    assert call(view=(0, 3, -1)) == -1 and 'member 2' in err()
    assert call(H=8, W=6, ow=6) == -1 and 'member 2' in err() and 'H == W' in err()      # view 5 is transposed
    assert call(H=8, W=6, ow=6, view=(0, 3, 1), null='logits') == -5                     # (the flips alone take any frame: only the null is refused)


def test_wrappers_refuse_host_tensors_and_unknown_names():
    z = torch.zeros((1, 1, 4, 4))
    out = torch.zeros((1, 4, 4, 4))
    with pytest.raises(ValueError, match='CUDA'):
        vote.vote_logits([z], [0], [0], out, 0)
    with pytest.raises(ValueError, match='mode'):
        vote.vote_logits([z], [0], [0], out, 0, mode='mean')
    with pytest.raises(ValueError, match='members'):
        vote.vote_logits([], [], [], out, 0, mode='soft')
    with pytest.raises(ValueError, match='CUDA'):
        vote.view_batch(z, 1)
    with pytest.raises(ValueError, match='uint8 CUDA tensor'):
        vote.segment_stack_voted(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [8, 8], ['Lumen'], 'models')
    with pytest.raises(ValueError, match='tta'):
        vote.segment_stack_voted([], [8, 8], ['Lumen'], 'models', tta='rot90')
    with pytest.raises(ValueError, match='mode'):
        vote.segment_stack_voted([], [8, 8], ['Lumen'], 'models', mode='mean')
    with pytest.raises(ValueError, match='no frames'):
        vote.segment_stack_voted([], [8, 8], ['Lumen'], 'models')


def test_predict_reads_the_three_keys_with_their_defaults():
    from oct_segmentation_amd.config import load_config
    from oct_segmentation_amd.predict import _vote_keys
    cfg = load_config('predict')
    assert 'folds' not in cfg and 'tta' not in cfg and 'vote' not in cfg                  # configs/predict.yaml stays the reference's
    assert _vote_keys(cfg) == (False, 'none', 'soft')
    assert _vote_keys(load_config('predict', ['folds=true', 'tta=d4', 'vote=majority'])) == (True, 'd4', 'majority')
    with pytest.raises(ValueError, match='tta'):
        _vote_keys({'tta': 'rot'})
    with pytest.raises(ValueError, match='vote'):
        _vote_keys({'vote': 'mean'})


def test_vote_report_layout():
    stats = torch.zeros((2, 4, 4), dtype=torch.int32)
    stats[0, 0] = torch.tensor([10, 4, 3, 5])
    stats[1, 3] = torch.tensor([0, 2, 0, 2])
    res = vote.VoteResult(None, None, None, stats, {'Lumen': 8, 'Vasa vasorum': 4})
    rep = vote.vote_report(res, ['a', 'b'], ['Lumen', 'Vasa vasorum'])
    assert rep['classes']['Lumen']['members'] == 8 and rep['classes']['Vasa vasorum']['members'] == 4
    assert rep['classes']['Lumen']['slices']['a'] == {'set': 10, 'disputed': 4, 'disputed_and_set': 3, 'dissent_sum': 5, 'disputed_ratio': 0.4}
    assert rep['classes']['Vasa vasorum']['slices']['b'] == {'set': 0, 'disputed': 2, 'disputed_and_set': 0, 'dissent_sum': 2, 'disputed_ratio': 2.0}
    assert json.loads(json.dumps(rep)) == rep
    with pytest.raises(ValueError, match='names'):
        vote.vote_report(res, ['a'], ['Lumen'])
