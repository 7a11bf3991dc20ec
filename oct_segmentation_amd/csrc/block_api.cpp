// block_api.cpp -- octseg_fpa_op / octseg_pab_op: one C-ABI door to each launcher of pan.hip's feature-pyramid-attention block (maxpool2,
// fpa_in_*, fpa_pyr_*, fpa_mix) and of pab.hip's position attention (pab_gemm, pab_softmax, pab_mix), so that every one can be pinned against
// a float64 reference alone (tests/test_gpu_blockops.py) instead of only through a whole PAN / MAnet.  A door of its own beside sweep_api.cpp:
// the pyramid alone takes more pointers than SweepSpec's 32-bit required-pointer mask can name.  An entry fills the launcher's arguments from
// a plain C descriptor and calls the launcher on the given stream; it refuses, before any launch, what the kernels cannot take.  Buffer sizes
// are the caller's contract (oct_segmentation_amd/blockops.py checks them): see include/octseg.h.
#include "plan_internal.h"

#include <initializer_list>

using namespace octseg;
using namespace octseg::detail;

namespace {

bool al(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool fits(long long v) { return v >= 1 && v < (1ll << 31); }
// the largest element index a [batch][rows][cols] walk with these strides reaches
size_t reach(int batch, size_t sb, int rows, size_t sr, int cols, size_t sc) { return (size_t)(batch - 1) * sb + (size_t)(rows - 1) * sr + (size_t)(cols - 1) * sc; }

}  // namespace

extern "C" {

size_t octseg_fpa_scratch_floats(int N, int H, int W) { return (N < 1 || H / 8 < 1 || W / 8 < 1) ? 0 : fpa_pyr_scratch_floats(N, H, W); }
size_t octseg_fpa_gscratch_floats(int N, int H, int W) { return (N < 1 || H / 8 < 1 || W / 8 < 1) ? 0 : fpa_pyr_gscratch_floats(N, H, W); }
size_t octseg_fpa_uu_offset(int N, int H, int W) { return (N < 1 || H / 8 < 1 || W / 8 < 1) ? 0 : fpa_pyr_uu_offset(N, H, W); }

int octseg_fpa_op(int stage, int dtype, const octseg_fpa_desc* d, void* stream) {
  static const char* const NAMES[OCTSEG_FPA_NUM_STAGES] = {"maxpool2_fwd", "maxpool2_bwd", "in_fwd", "in_bwd", "pyr_fwd", "pyr_bwd", "mix_fwd", "mix_bwd"};
  if (stage < 0 || stage >= OCTSEG_FPA_NUM_STAGES) return fail(OCTSEG_BAD_ARG, "fpa_op: unknown stage");
  const std::string who = std::string("fpa_op ") + NAMES[stage] + ": ";
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  const bool train_only = stage == OCTSEG_FPA_MAXPOOL2_BWD || stage == OCTSEG_FPA_IN_BWD || stage == OCTSEG_FPA_PYR_BWD || stage == OCTSEG_FPA_MIX_BWD;
  if (dtype == OCTSEG_F16 && train_only) return fail(OCTSEG_BAD_DTYPE, who + "a training-only stage has no f16 form (f16 is the serving dtype)");
  if (d == nullptr) return bad_arg("null descriptor");
  const size_t el = dtype == OCTSEG_F32 ? 4 : 2;
  const int vec = ev_vec(dtype);
  hipStream_t st = (hipStream_t)stream;
  if (d->N < 1 || d->H < 1 || d->W < 1) return bad_shape("empty tensor");
  const long long npix = (long long)d->N * d->H * d->W;

  switch (stage) {
    case OCTSEG_FPA_MAXPOOL2_FWD: case OCTSEG_FPA_MAXPOOL2_BWD: {
      const bool bwd = stage == OCTSEG_FPA_MAXPOOL2_BWD;
      if (d->C < 1 || d->C % vec != 0) return bad_shape("C is not a whole number of 16-byte vectors");
      if ((d->H & 1) || (d->W & 1)) return bad_shape("odd H or W");
      if (!fits(npix * d->C)) return bad_shape("tensor of 2^31 elements or more");
      if (d->x == nullptr || (bwd ? (d->dp == nullptr || d->dx == nullptr) : d->p == nullptr)) return bad_arg("null required pointer");
      if (!al(d->x, 16) || (bwd ? (!al(d->dp, 16) || !al(d->dx, 16)) : !al(d->p, 16))) return bad_arg("the tensors of the vector kernel must be 16-byte aligned");
      if (bwd) HIPCHK(launch_maxpool2(dtype, d->x, nullptr, d->dp, d->dx, d->N, d->H, d->W, d->C, d->accum ? 1 : 0, st));
      else HIPCHK(launch_maxpool2(dtype, d->x, d->p, nullptr, nullptr, d->N, d->H, d->W, d->C, 0, st));
      return OCTSEG_OK;
    }
    case OCTSEG_FPA_IN_FWD: case OCTSEG_FPA_IN_BWD: {
      const bool bwd = stage == OCTSEG_FPA_IN_BWD;
      if (d->C < 1) return bad_shape("empty tensor");
      if (d->K < 1 || d->K > 15 || !(d->K & 1)) return bad_shape("K must be odd and at most 15");
      if (!fits(npix * d->C)) return bad_shape("tensor of 2^31 elements or more");
      if (d->p == nullptr || d->w == nullptr) return bad_arg("null required pointer");
      if (bwd ? (d->dy == nullptr || d->dp == nullptr || d->dw == nullptr || d->db == nullptr) : (d->b == nullptr || d->y == nullptr)) return bad_arg("null required pointer");
      if (!al(d->p, el) || !al(d->dp, el) || !al(d->w, 4) || !al(d->b, 4) || !al(d->y, 4) || !al(d->dy, 4) || !al(d->dw, 4) || !al(d->db, 4))
        return bad_arg("a pointer is not aligned to its element");
      if (bwd) HIPCHK(launch_fpa_in_bwd(dtype, d->p, d->dy, d->w, d->dp, d->dw, d->db, d->N, d->H, d->W, d->C, d->K, st));
      else HIPCHK(launch_fpa_in_fwd(dtype, d->p, d->w, d->b, d->y, d->N, d->H, d->W, d->C, d->K, st));
      return OCTSEG_OK;
    }
    case OCTSEG_FPA_PYR_FWD: case OCTSEG_FPA_PYR_BWD: {
      const bool bwd = stage == OCTSEG_FPA_PYR_BWD;
      if (d->H / 8 < 1 || d->W / 8 < 1) return bad_shape("the pyramid needs H / 8 >= 1 and W / 8 >= 1");
      if (!fits(npix)) return bad_shape("tensor of 2^31 elements or more");
      const int train = bwd ? 1 : (d->train ? 1 : 0);
      if (train && (long long)d->N * (d->H / 8) * (d->W / 8) <= 1) {   // the plan's own refusal (plan_forward.cpp run_forward), as torch raises it
        char buf[192];
        snprintf(buf, sizeof buf, "Expected more than 1 value per channel when training, got input size torch.Size([%d, %d, %d, %d])", d->N, 1, d->H / 8, d->W / 8);
        return fail(OCTSEG_BAD_SHAPE, buf);
      }
      if (d->scratch == nullptr || (bwd && (d->gscratch == nullptr || d->duu == nullptr))) return bad_arg("null required pointer");
      if (!al(d->scratch, 4) || !al(d->gscratch, 4) || !al(d->duu, 4)) return bad_arg("a pointer is not aligned to its element");
      if (d->scratch_floats < fpa_pyr_scratch_floats(d->N, d->H, d->W)) return bad_arg("scratch smaller than fpa_pyr_scratch_floats");
      if (bwd && d->gscratch_floats < fpa_pyr_gscratch_floats(d->N, d->H, d->W)) return bad_arg("gscratch smaller than fpa_pyr_gscratch_floats");
      FpaPyrArgs a;
      memset(&a, 0, sizeof(a));
      a.N = d->N; a.h = d->H; a.w = d->W; a.train = train; a.scratch = d->scratch;
      if (bwd) { a.gscratch = d->gscratch; a.duu = d->duu; }
      for (int l = 0; l < 6; ++l) {
        // layer 0's conv is fpa_in_*: the pyramid reads no weight, bias or their gradients of it
        const bool conv = l >= 1;
        if ((conv && d->pw[l] == nullptr) || d->pg[l] == nullptr) return bad_arg("null required pointer");
        if (!bwd && ((conv && d->pb[l] == nullptr) || d->pbe[l] == nullptr || d->prm[l] == nullptr || d->prv[l] == nullptr)) return bad_arg("null required pointer");
        if (bwd && ((conv && (d->pdw[l] == nullptr || d->pdb[l] == nullptr)) || d->pdg[l] == nullptr || d->pdbe[l] == nullptr)) return bad_arg("null required pointer");
        if (!al(d->pw[l], 4) || !al(d->pb[l], 4) || !al(d->pg[l], 4) || !al(d->pbe[l], 4) || !al(d->prm[l], 4) || !al(d->prv[l], 4) || !al(d->pdw[l], 4) ||
            !al(d->pdb[l], 4) || !al(d->pdg[l], 4) || !al(d->pdbe[l], 4))
          return bad_arg("a pointer is not aligned to its element");
        a.w_[l] = d->pw[l]; a.b_[l] = d->pb[l]; a.g_[l] = d->pg[l]; a.be_[l] = d->pbe[l];
        if (!bwd) { a.rm_[l] = d->prm[l]; a.rv_[l] = d->prv[l]; }
        else { a.dw_[l] = d->pdw[l]; a.db_[l] = d->pdb[l]; a.dg_[l] = d->pdg[l]; a.dbe_[l] = d->pdbe[l]; }
      }
      if (bwd) HIPCHK(launch_fpa_pyr_bwd(a, st));
      else HIPCHK(launch_fpa_pyr_fwd(a, st));
      return OCTSEG_OK;
    }
    case OCTSEG_FPA_MIX_FWD: case OCTSEG_FPA_MIX_BWD: {
      const bool bwd = stage == OCTSEG_FPA_MIX_BWD;
      if (d->C < 1) return bad_shape("empty tensor");
      if (!fits(npix * d->C)) return bad_shape("tensor of 2^31 elements or more");
      if (d->uu == nullptr || d->mid == nullptr) return bad_arg("null required pointer");
      if (bwd ? (d->g == nullptr || d->dmid == nullptr || d->duu == nullptr) : (d->b1 == nullptr || d->out == nullptr)) return bad_arg("null required pointer");
      if (!al(d->uu, 4) || !al(d->duu, 4) || !al(d->mid, el) || !al(d->b1, el) || !al(d->out, el) || !al(d->g, el) || !al(d->dmid, el))
        return bad_arg("a pointer is not aligned to its element");
      if (bwd) HIPCHK(launch_fpa_mix(dtype, d->uu, d->mid, nullptr, nullptr, d->g, d->dmid, d->duu, d->N, d->H * d->W, d->C, st));
      else HIPCHK(launch_fpa_mix(dtype, d->uu, d->mid, d->b1, d->out, nullptr, nullptr, nullptr, d->N, d->H * d->W, d->C, st));
      return OCTSEG_OK;
    }
  }
  return bad_arg("unknown stage");
}

int octseg_pab_op(int stage, int dtype, const octseg_pab_desc* d, void* stream) {
  static const char* const NAMES[OCTSEG_PAB_NUM_STAGES] = {"gemm", "softmax_fwd", "softmax_bwd", "mix_fwd", "mix_bwd"};
  if (stage < 0 || stage >= OCTSEG_PAB_NUM_STAGES) return fail(OCTSEG_BAD_ARG, "pab_op: unknown stage");
  const std::string who = std::string("pab_op ") + NAMES[stage] + ": ";
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  if (dtype == OCTSEG_F16 && (stage == OCTSEG_PAB_SOFTMAX_BWD || stage == OCTSEG_PAB_MIX_BWD))
    return fail(OCTSEG_BAD_DTYPE, who + "a training-only stage has no f16 form (f16 is the serving dtype)");
  if (d == nullptr) return bad_arg("null descriptor");
  const size_t el = dtype == OCTSEG_F32 ? 4 : 2;
  hipStream_t st = (hipStream_t)stream;

  switch (stage) {
    case OCTSEG_PAB_GEMM: {
      const octseg_pab_gemm& s = d->gemm;
      if (s.M < 1 || s.N < 1 || s.K < 1 || s.batch < 1) return bad_shape("empty product");
      if (s.batch > 65535) return bad_shape("batch > 65535 (a grid dimension)");
      if ((s.M + 15) / 16 > 65535) return bad_shape("more than 65535 row tiles (a grid dimension)");
      if (s.A == nullptr || s.B == nullptr || s.C == nullptr) return bad_arg("null required pointer");
      if (!al(s.A, s.a_f32 ? 4 : el) || !al(s.B, s.b_f32 ? 4 : el) || !al(s.C, s.c_f32 ? 4 : el)) return bad_arg("a pointer is not aligned to its element");
      for (size_t v : {s.sAb, s.sAm, s.sAk, s.sBb, s.sBk, s.sBn, s.sCb, s.sCm, s.sCn})
        if (v >= ((size_t)1 << 31)) return bad_shape("a stride of 2^31 elements or more");
      if (reach(s.batch, s.sAb, s.M, s.sAm, s.K, s.sAk) >= d->numelA) return bad_shape("the largest reachable index of A lies beyond numelA");
      if (reach(s.batch, s.sBb, s.K, s.sBk, s.N, s.sBn) >= d->numelB) return bad_shape("the largest reachable index of B lies beyond numelB");
      if (reach(s.batch, s.sCb, s.M, s.sCm, s.N, s.sCn) >= d->numelC) return bad_shape("the largest reachable index of C lies beyond numelC");
      PabGemm g;
      memset(&g, 0, sizeof(g));
      g.A = s.A; g.B = s.B; g.C = s.C;
      g.sAb = s.sAb; g.sAm = s.sAm; g.sAk = s.sAk; g.sBb = s.sBb; g.sBk = s.sBk; g.sBn = s.sBn; g.sCb = s.sCb; g.sCm = s.sCm; g.sCn = s.sCn;
      g.M = s.M; g.N = s.N; g.K = s.K; g.batch = s.batch; g.a_f32 = s.a_f32; g.b_f32 = s.b_f32; g.c_f32 = s.c_f32; g.accum = s.accum;
      HIPCHK(launch_pab_gemm(dtype, g, st));
      return OCTSEG_OK;
    }
    case OCTSEG_PAB_SOFTMAX_FWD: case OCTSEG_PAB_SOFTMAX_BWD: {
      const bool bwd = stage == OCTSEG_PAB_SOFTMAX_BWD;
      if (d->n == 0) return bad_shape("n == 0");
      if (d->batch < 1) return bad_shape("empty batch");
      if (d->batch > 65535) return bad_shape("batch > 65535");
      if (d->n >= ((size_t)1 << 31) / (size_t)d->batch) return bad_shape("tensor of 2^31 elements or more");
      if (d->S == nullptr || (bwd && d->P == nullptr)) return bad_arg("null required pointer");
      if (!al(d->S, 4) || !al(d->P, 4)) return bad_arg("a pointer is not aligned to its element");
      HIPCHK(launch_pab_softmax(d->S, bwd ? d->P : nullptr, d->batch, d->n, bwd ? 1 : 0, st));
      return OCTSEG_OK;
    }
    case OCTSEG_PAB_MIX_FWD: case OCTSEG_PAB_MIX_BWD: {
      const bool bwd = stage == OCTSEG_PAB_MIX_BWD;
      if (d->N < 1 || d->HW < 1 || d->C < 1) return bad_shape("empty tensor");
      if (!fits((long long)d->N * d->HW * d->C)) return bad_shape("tensor of 2^31 elements or more");
      if (bwd ? (d->dy == nullptr || d->dM == nullptr) : (d->x == nullptr || d->M == nullptr || d->y == nullptr)) return bad_arg("null required pointer");
      if (!al(d->x, el) || !al(d->y, el) || !al(d->dy, el) || !al(d->M, 4) || !al(d->dM, 4)) return bad_arg("a pointer is not aligned to its element");
      if (bwd) HIPCHK(launch_pab_mix(dtype, nullptr, nullptr, nullptr, d->dM, d->dy, d->N, d->HW, d->C, st));
      else HIPCHK(launch_pab_mix(dtype, d->x, d->M, d->y, nullptr, nullptr, d->N, d->HW, d->C, st));
      return OCTSEG_OK;
    }
  }
  return bad_arg("unknown stage");
}

}  // extern "C"
