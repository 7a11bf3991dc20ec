"""Element-wise parity of augment_kernel (csrc/augment.hip, through octseg_augment) with its float64 restatement tests/augment_kernel_ref.py.

One launch per case; the cases and their caps are listed in tests/augment_cases.py, the rules that turn a float64 value into one value or
two candidates in tests/augment_kernel_ref.py, and tests/test_augment_kernel.py anchors the restatement on the CPU.  img, mask, params, img_out
and mask_out are interior views of larger allocations with 4 KiB NaN margins either side; the outputs start as NaN; after each call every
margin must be untouched and every output element finite.  Rule X cases (exact, stride) are compared with torch indexing bit for bit AND with
the restatement; everywhere else every element must be one of its candidates, open pixels must stay on the output grid, and the share of
two-valued and open pixels must stay inside the family's cap.  Non-square frames test the kernel, not the sampler.

What a defect in the kernel looks like here (each was put into a scratch copy of augment.hip, never committed): see MUTATIONS below.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_kernel_ref as KR
import sweep_ref as R
from oct_segmentation_amd import _lib as L

pytestmark = pytest.mark.gpu

MEASURED = """
MI355X, the "SHARES" and "RATIO" lines of the run.  Every element of every case was one of its candidates; exact and stride also equal torch
indexing bit for bit.  Share of pixels that are two-valued (any channel) | open, image; two-valued, mask (the restatement's own figures: the
kernel cannot change them; caps in augment_cases.py):
  warp 64 x 64      0.179 % | 0        mask 0           warp 48 x 80      0.204 % | 0        mask 0            (cap 1 %, 0.1 %)
  cropwarp 64 x 64  0.165 % | 0        mask 0           cropwarp 48 x 80  0.150 % | 0        mask 0            (cap 1 %, 0.1 %)
  chain 200 x 64^2  0.093 % | 0.023 %  mask 0.0001 %    (617 rounding ties, 318 HSV ties, 17 noise boundaries; cap 1 %, 0.1 %)
  hsv round trip    0.816 % | 0                         hsv shifts        0.884 % | 0                          (cap 2 %)
  bc                0.0061 % of the entries (3 of 49152; cap 0.2 %)       noise   0.0719 % of the elements (53 of 73728; cap 0.1 %)
  exact, stride     0
Noise, kernel against the float32 yardstick (numpy on the CPU; its largest distance from float64 per frame is 1.53e-5 .. 1.57e-5 at sigma >= 1.2
and 7.6e-6 at sigma 0.01: the rounding of the sum at 255): needed 0.000 x the yardstick (the kernel floors every one of the 73728 elements as float64 does; allowed 4, or
the Rule E floor), and it resolved elements as close as 0.096 x the yardstick to an integer.
The file runs in about 3.5 s (stride 1.6 s, hsv 0.9 s, chain 0.5 s, bc 0.4 s: mostly the restatement on the CPU, computed once per case).
"""

MUTATIONS = """
One-line changes to augment.hip, each built into a scratch copy of the library and run once (MI355X); none is committed.  "old" = tests/test_augment.py.
  floorf(sx + 0.5f) -> floorf(sx) in the mask gather          red: exact, warp, cropwarp, chain            old: green
  xx < W -> xx < H in `at`                                     red: exact, warp, cropwarp, the ABI run      old: green (every frame there is square)
  hash3(seed, i, 2u * c) -> hash3(seed, i, 0u) for u1          red: noise, chain                            old: green
  the crop test on sx, sy instead of cx, cy                    red: exact, warp, cropwarp, chain            old: red (2 tests)
  (hh * hdiv + 2048) >> 12 -> (hh * hdiv) >> 12                red: hsv, chain                              old: red (2 tests)
"""

BAD_SHAPE, BAD_ARG = -1, -5      # include/octseg.h; octseg_augment in csrc/api.cpp: null pointer or aliased output BAD_ARG, an extent <= 0 BAD_SHAPE


def _call(img, mask, img_out, mask_out, params, B, Cn, H, W):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    return L.lib().octseg_augment(p(img), p(mask), p(img_out), p(mask_out), p(params), B, Cn, H, W, L.stream_ptr())


def run_case(case, dev):
    """-> (failures, share of two-valued / open pixels taken by the kernel's answer, noise ratio or None)."""
    B, _, H, W = case.img.shape
    Cn = case.mask.shape[1]
    G = R.Guard(dev)
    img, mask, params = G.put(case.img), G.put(case.mask), G.put(torch.from_numpy(case.params))
    img_out, mask_out = G.empty(case.img.shape, torch.float32), G.empty(case.mask.shape, torch.float32)
    L.check(_call(img, mask, img_out, mask_out, params, B, Cn, H, W))
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(img.cpu(), case.img) and torch.equal(mask.cpu(), case.mask), 'an input changed'
    got_i, got_m = img_out.cpu().numpy(), mask_out.cpu().numpy()
    fails = []
    if case.expect is not None:
        for name, got, want in (('img', got_i, case.expect[0].numpy()), ('mask', got_m, case.expect[1].numpy())):
            if not np.array_equal(got.view(np.int32), want.view(np.int32)):
                bad = got.view(np.int32) != want.view(np.int32)
                i = tuple(int(t[0]) for t in np.nonzero(bad))
                fails.append(f'{name}: {int(bad.sum())} of {bad.size} elements differ from torch indexing; first at {i}: got {got[i]!r}, want {want[i]!r}')
    res = case.ref()
    fails += KR.compare(res, got_i, got_m)
    if res.uncertain_img(case.unit) > case.cap_img or res.uncertain_mask() > case.cap_mask:
        fails.append(f'cap: image {res.uncertain_img(case.unit):.5f} > {case.cap_img} or mask {res.uncertain_mask():.5f} > {case.cap_mask}')
    ratio = None
    if case.id.startswith('noise') and not fails:
        # The kernel returns floor(px + n), not px + n, so its distance from float64 shows only where it crosses an integer: `needed` = the
        # farthest px + n had to move to land where the kernel put it (0: the kernel floors every element as float64 does), `resolved` = how
        # close to an integer the nearest element was that it still floored as float64 does; both in units of the float32 yardstick's distance
        needed, resolved = 0.0, np.inf
        for n in np.nonzero(res.noise_yard)[0]:
            s = res.noise_sum[n]
            f = np.floor(np.clip(s, 0.0, 255.0))
            up, down = got_i[n] > f, got_i[n] < f
            needed = max(needed, float(np.where(up, got_i[n] - s, np.where(down, s - f, 0.0)).max()) / res.noise_yard[n])
            free = (got_i[n] == f) & (s > 0.0) & (s < 255.0) & (res.noise[n] != 0.0)
            resolved = min(resolved, float(np.minimum(s - np.floor(s), np.ceil(s) - s)[free].min()) / res.noise_yard[n])
        ratio = (needed, resolved)
    return fails, res.shares(), ratio


@pytest.mark.parametrize('family', sorted(AC.FAMILIES))
def test_augment_family(family, cuda):
    """Every case of the family runs (a failure does not hide the ones behind it); the report names each failing case."""
    failures = []
    cases = AC.FAMILIES[family]()
    for case in cases:
        try:
            fails, shares, ratio = run_case(case, cuda)
            failures += [f'{case.id}: {f[:400]}' for f in fails]
            if family not in ('exact',):
                print(f'SHARES {case.id}: ' + ' '.join(f'{k} {100 * v:.4f}%' for k, v in shares.items()))
            if ratio is not None:
                print(f'RATIO noise kernel / float32 yardstick: needed {ratio[0]:.3f} (allowed 4, or the Rule E floor), resolved down to {ratio[1]:.3f}')
        except AssertionError as e:
            failures.append(f'{case.id}: {str(e)[:400]}')
        except Exception as e:
            if isinstance(e, RuntimeError) and ('HIP' in str(e) or 'octseg error -4' in str(e)):      # a HIP error: nothing more is started on this GPU
                pytest.exit(f'{case.id}: {e!r}', returncode=3)
            failures.append(f'{case.id}: {e!r}'[:400])
    assert not failures, f'{len(failures)} failures in {len(cases)} cases:\n' + '\n'.join(failures)


def test_abi_refusals_leave_the_outputs_untouched(cuda):
    """Null pointers, B, classes, H or W <= 0 and an output that aliases its input return the documented code; nothing is launched."""
    B, Cn, H, W = 2, 3, 5, 7
    G = R.Guard(cuda)
    img, mask = G.put(torch.ones(B, 3, H, W)), G.put(torch.ones(B, Cn, H, W))
    params = G.put(torch.from_numpy(np.stack([AC.row(), AC.row()])))
    img_out, mask_out = G.empty((B, 3, H, W), torch.float32), G.empty((B, Cn, H, W), torch.float32)
    full = [img, mask, img_out, mask_out, params]
    for k in range(5):
        a = list(full)
        a[k] = None
        assert _call(*a, B, Cn, H, W) == BAD_ARG, k
    for k in range(4):
        dims = [B, Cn, H, W]
        for bad in (0, -1):
            dims[k] = bad
            assert _call(*full, *dims) == BAD_SHAPE, (k, bad)
    assert _call(img_out, mask, img_out, mask_out, params, B, Cn, H, W) == BAD_ARG        # img_out == img
    assert _call(img, mask_out, img_out, mask_out, params, B, Cn, H, W) == BAD_ARG        # mask_out == mask
    torch.cuda.synchronize()
    G.check()
    assert bool(torch.isnan(img_out).all()) and bool(torch.isnan(mask_out).all())
    assert bool((img == 1).all()) and bool((mask == 1).all())
    L.check(_call(*full, B, Cn, H, W))                                                    # the same buffers, well-formed: runs
    torch.cuda.synchronize()
    G.check()
    assert bool((img_out == 1).all()) and bool((mask_out == 1).all())
