// plan_dryrun.cpp -- host-only walk of the plan builder under AddressSanitizer + UBSan ("race detection / sanitizers").
//
// Built by `make -C oct_segmentation_amd/csrc asan` from the HOST halves of every source (hipcc --cuda-host-only
// -fsanitize=address,undefined): graph construction, workspace layout, tap tables, launch geometry, weight-image layouts, BN slab row
// counts and the one-launch pack / BN job tables of csrc/plan_geom.cpp and csrc/plan_build.cpp -- ~1400 lines of index arithmetic -- run for every architecture x
// encoder pair at the smallest legal frame, the benchmark frame and a non-square one, in all three dtypes, with no kernel launched
// (no GPU needed).  A subset of the plans is then driven through octseg_net_forward / _backward / _backward_sliced / octseg_optim_step and
// the graph-captured eval forward, and the class-activation-map path (frozen forward, seeded backward, map launches) against tools/hip_host_stubs.cpp, a recording stand-in for the HIP runtime that checks every launch
// geometry and every memset / copy range; the boundary-distance entry points (csrc/distance.hip), the 3-D lesion entry points (csrc/lesions.hip), the lesion-matching entry points (csrc/match.hip) and the
// mask clean-up entry points (csrc/components.hip) are driven the same way, from a 1 x 1 frame to the largest one each takes.  Exit code 0 = the sanitizers and the stubs saw nothing.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/octseg.h"

// tools/hip_host_stubs.cpp: the recording HIP stand-in this binary links instead of libamdhip64
extern "C" void dry_register_range(const void* lo, size_t bytes);
extern "C" void dry_clear_ranges();
extern "C" unsigned long long dry_launches();
extern "C" unsigned long long dry_memops();
extern "C" unsigned long long dry_errors();
extern "C" unsigned long long dry_fingerprint();

namespace {
int g_slices_seen = 0;
size_t g_slice_cover = 0;
void slice_cb(void*, int, size_t b, size_t e) { ++g_slices_seen; g_slice_cover += e - b; }

// One training step + eval forwards of a plan with every pointer inside fake, registered address ranges (never dereferenced: all device
// work is behind the stubs).  Walks run_forward / run_backward: source and destination descriptors, launch routing, split-K geometry,
// slab rows, stream forks and joins, slice bookkeeping.
int exercise(const octseg_net_desc& d, octseg_plan* p) {
  char* base = (char*)(uintptr_t)0x100000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  dry_clear_ranges();
  const size_t np = octseg_plan_param_numel(p), nb = octseg_plan_buffer_numel(p), ws = octseg_plan_workspace_bytes(p);
  const size_t px = (size_t)d.batch * d.height * d.width;
  float* params = (float*)carve(np * 4); float* grads = (float*)carve(np * 4); float* bufs = (float*)carve(nb * 4);
  float* m = (float*)carve(np * 4); float* v = (float*)carve(np * 4);
  void* wsp = carve(ws);
  float* image = (float*)carve(px * 3 * 4); float* logits = (float*)carve(px * d.classes * 4); float* target = (float*)carve(px * d.classes * 4);
  float* loss = (float*)carve(4); long long* stats = (long long*)carve((size_t)d.batch * d.classes * 4 * 8);
  const int dls = !strcmp(d.arch, "deeplabv3plus") ? 16 : !strcmp(d.arch, "deeplabv3") ? 8 : 0;   // element-wise [B][H/s][W/s][256]; fpn [B][128], pspnet [B][512]
  float* keep = (float*)carve(dls ? (size_t)d.batch * (d.height / dls) * (d.width / dls) * 256 * 4 : (size_t)d.batch * 512 * 4);
  octseg_plan_set_dropout(p, keep);                 // (ignored by the other architectures)
  float* dcf = (float*)carve((size_t)(octseg_plan_num_drop_connect(p) + 1) * d.batch * 4);
  octseg_plan_set_drop_connect(p, dcf);             // EfficientNet encoders: drop_connect factors of the id skips
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  void* st = (void*)(uintptr_t)0x4000; void* comm = (void*)(uintptr_t)0x4100;
  const unsigned long long l0 = dry_launches();
  if (d.dtype != OCTSEG_F16) {
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 1, mean, stdv, 1, st) != 0) { fprintf(stderr, "forward: %s\n", octseg_last_error()); return 10; }
    if (octseg_dice_forward(p, wsp, logits, target, loss, stats, st) != 0) return 11;
    if (octseg_net_backward(p, params, grads, wsp, logits, target, 1.0f, st) != 0) { fprintf(stderr, "backward: %s\n", octseg_last_error()); return 12; }
    for (int ns : {1, 3, 7}) {
      g_slices_seen = 0; g_slice_cover = 0;
      if (octseg_net_backward_sliced(p, params, grads, wsp, logits, target, 0.5f, st, ns, comm, slice_cb, nullptr) != 0) return 13;
      if (g_slice_cover != np || g_slices_seen < 1 || g_slices_seen > ns) { fprintf(stderr, "slices do not tile the arena (%d slices, %zu of %zu)\n", g_slices_seen, g_slice_cover, np); return 14; }
    }
    for (int kind = 0; kind < 4; ++kind)
      if (octseg_optim_step(kind, params, grads, m, v, np, 1e-3f, 1e-4f, 1, 1.0f, st) != 0) return 15;
    octseg_plan_params_changed(p);
    octseg_debug_set_serial(1);                      // the one-stream measurement mode takes other branches
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 1, mean, stdv, 1, st) != 0) return 16;
    if (octseg_net_backward(p, params, grads, wsp, logits, target, 1.0f, st) != 0) return 16;
    octseg_debug_set_serial(0);
    octseg_set_deterministic(1);                     // ... and so does the deterministic-reduction mode
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 1, mean, stdv, 1, st) != 0) return 17;
    if (octseg_dice_forward(p, wsp, logits, target, loss, nullptr, st) != 0) return 17;
    if (octseg_net_backward(p, params, grads, wsp, logits, target, 1.0f, st) != 0) return 17;
    octseg_set_deterministic(0);
  } else {
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 1, mean, stdv, 1, st) == 0) return 18;      // f16 trains nowhere
    if (octseg_net_backward(p, params, grads, wsp, logits, target, 1.0f, st) == 0) return 18;
  }
  if (octseg_net_forward(p, params, bufs, wsp, image, logits, 0, nullptr, nullptr, 0, st) != 0) { fprintf(stderr, "eval forward: %s\n", octseg_last_error()); return 19; }
  octseg_plan_set_graph(p, 1);                       // eager call, capture, replay
  for (int k = 0; k < 3; ++k)
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 0, nullptr, nullptr, 0, st) != 0) return 20;
  octseg_plan_set_graph(p, 0);
  if (dry_launches() - l0 < 50) { fprintf(stderr, "suspiciously few launches\n"); return 21; }
  // class activation maps: the frozen-BatchNorm forward, the seeded data-only backward (null gradient arena) and the map launches on the
  // target tensor, where the pair is built; every other pair must refuse the mode
  const int frc = octseg_plan_set_frozen_bn(p, 1);
  if (frc == 0) {
    size_t ao = 0, go = 0; int dm[4] = {0, 0, 0, 0};
    if (octseg_plan_cam_target(p, &ao, &go, dm) != 0) return 22;
    const size_t bytes = (size_t)dm[0] * dm[1] * dm[2] * dm[3] * (d.dtype == OCTSEG_F32 ? 4 : 2);
    if (dm[0] != d.batch || ao + bytes > ws || go + bytes > ws) { fprintf(stderr, "the CAM target leaves the workspace\n"); return 22; }
    if (octseg_net_forward(p, params, bufs, wsp, image, logits, 1, mean, stdv, 1, st) != 0) { fprintf(stderr, "frozen forward: %s\n", octseg_last_error()); return 23; }
    if (octseg_net_backward_seeded(p, params, wsp, target, st) != 0) { fprintf(stderr, "seeded backward: %s\n", octseg_last_error()); return 24; }
    const int S = d.height;
    void* scratch = carve(octseg_cam_scratch_bytes(dm[0], dm[1], dm[2], dm[3]));
    float* maps = (float*)carve((size_t)dm[0] * S * S * 4);
    uint8_t* bin = (uint8_t*)carve((size_t)dm[0] * S * S); uint8_t* ov = (uint8_t*)carve((size_t)dm[0] * S * S * 3);
    uint8_t* gt = (uint8_t*)carve((size_t)dm[0] * 75 * 50); int* rows = (int*)carve(75 * 4); int* cols = (int*)carve(50 * 4); int* counts = (int*)carve((size_t)dm[0] * 12);
    float* frames = (float*)carve((size_t)dm[0] * 3 * S * S * 4); uint8_t* jet = (uint8_t*)carve(768);
    for (int method = 0; method < 6; ++method)
      if (octseg_cam_maps(d.dtype, (char*)wsp + ao, (char*)wsp + go, dm[0], dm[1], dm[2], dm[3], method, S, scratch, maps, 0.5f, bin, gt, 75, 50, rows, cols,
                          counts, frames, jet, 0.5, ov, st) != 0) { fprintf(stderr, "cam_maps: %s\n", octseg_last_error()); return 25; }
    if (octseg_cam_overlay(maps, frames, jet, dm[0], S, 0.5, ov, scratch, st) != 0) return 25;
    octseg_plan_set_frozen_bn(p, 0);
  } else if (frc != OCTSEG_UNSUPPORTED_ARCH && frc != OCTSEG_BAD_DTYPE) {
    return 26;
  }
  return 0;
}

// The boundary-distance entry points (csrc/distance.hip, csrc/distance_api.cpp) against the stubs: the scratch carving, the three memsets
// (non-empty flags, slot cursors, minima) inside their ranges and every grid, from a 1 x 1 frame to the largest one the calls take; then
// what they must refuse.
int exercise_distance() {
  char* base = (char*)(uintptr_t)0x200000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 97, 130, 5}, {186, 750, 750, 4}, {2, 4096, 4096, 16}};
  const int P = 7;
  for (auto& sh : shapes) {
    dry_clear_ranges();
    const int N = sh[0], H = sh[1], W = sh[2], C = sh[3];
    const size_t one = octseg_distance_scratch_bytes(N, H, W, C, 0, 0), two = octseg_distance_scratch_bytes(N, H, W, C, C, P);
    if (one == 0 || two <= one) return 30;
    const size_t elems = (size_t)N * H * W * C;
    float* a = (float*)carve(elems * 4);
    float* b = (float*)carve(elems * 4);
    float* out = (float*)carve(elems * 4);
    int* d2 = (int*)carve(elems * 4);
    void* scratch = carve(two);
    int* pairs = (int*)carve(P * 2 * 4);
    int* counts = (int*)carve((size_t)N * P * 2 * 4);
    int* overlap = (int*)carve((size_t)N * P * 3 * 4);
    long long* offsets = (long long*)carve((size_t)N * P * 8);
    long long* keys = (long long*)carve(1024 * 8);
    int* overflow = (int*)carve(4);
    unsigned long long* minima = (unsigned long long*)carve((size_t)N * P * 8);
    void* st = (void*)(uintptr_t)0x5000;
    if (octseg_stack_boundary(a, N, H, W, C, scratch, one, out, st) != 0) { fprintf(stderr, "stack_boundary: %s\n", octseg_last_error()); return 31; }
    for (int to = 0; to < 3; ++to)
      if (octseg_stack_distance(a, N, H, W, C, to, scratch, one, d2, st) != 0) { fprintf(stderr, "stack_distance: %s\n", octseg_last_error()); return 32; }
    if (octseg_pair_distance_counts(a, b, N, H, W, C, C, pairs, P, 2, 2, scratch, two, counts, overlap, st) != 0) return 33;
    if (octseg_pair_distance_counts(a, a, N, H, W, C, C, pairs, P, 0, 1, scratch, two, counts, nullptr, st) != 0) return 33;
    if (octseg_pair_distance_keys(a, b, N, H, W, C, C, pairs, P, 2, 2, scratch, two, 5, offsets, keys, 1024, overflow, st) != 0) return 34;
    if (octseg_pair_distance_min(a, b, N, H, W, C, C, pairs, P, 0, 0, scratch, two, minima, st) != 0) return 35;
    // refused before anything is enqueued
    const unsigned long long before = dry_launches() + dry_memops();
    if (octseg_stack_distance(a, N, H, W, C, 0, scratch, one - 1, d2, st) == 0 || octseg_stack_distance(a, N, H, 4097, C, 0, scratch, one, d2, st) == 0 ||
        octseg_stack_distance(a, N, H, W, 17, 0, scratch, one, d2, st) == 0 || octseg_stack_distance(a, N, H, W, C, 3, scratch, one, d2, st) == 0 ||
        octseg_stack_boundary(a, N, H, W, C, scratch, one, a, st) == 0 ||
        octseg_pair_distance_counts(a, b, N, H, W, C, C, pairs, P, 2, 2, scratch, two - 1, counts, overlap, st) == 0 ||
        octseg_pair_distance_keys(a, b, N, H, W, C, C, pairs, P, 2, 2, scratch, two, 0, offsets, keys, 0, overflow, st) == 0 ||
        octseg_pair_distance_keys(a, b, N, H, W, C, C, pairs, P, 2, 2, scratch, two, (1ll << 31) - 1, offsets, keys, 1024, overflow, st) == 0 ||
        octseg_pair_distance_min(a, b, N, H, W, C, C, pairs, 0, 0, 0, scratch, two, minima, st) == 0)
      return 36;
    if (dry_launches() + dry_memops() != before) { fprintf(stderr, "a refused distance call enqueued work\n"); return 37; }
  }
  if (octseg_distance_scratch_bytes(1, 4097, 8, 1, 0, 0) != 0 || octseg_distance_scratch_bytes(1, 8, 8, 17, 0, 0) != 0) return 38;
  return 0;
}

// The 3-D lesion entry points (csrc/lesions.hip, csrc/lesions_api.cpp) against the stubs: the scratch carving, the two memsets (lesion counters,
// profile) inside their ranges and every grid, from a single voxel to a volume just under 2^31 - 1 voxels; then what they must refuse.
int exercise_lesions() {
  char* base = (char*)(uintptr_t)0x300000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  const int shapes[][4] = {{1, 1, 1, 1}, {5, 97, 130, 5}, {186, 750, 750, 4}, {2047, 1024, 1024, 16}};
  for (auto& sh : shapes) {
    dry_clear_ranges();
    const int N = sh[0], H = sh[1], W = sh[2], C = sh[3];
    const size_t need = octseg_lesions_scratch_bytes(C, N, H, W);
    if (need == 0 || need <= octseg_lesions_scratch_bytes(1, N, H, W) - (C == 1)) return 40;
    const size_t elems = (size_t)N * H * W * C;
    float* a = (float*)carve(elems * 4);
    float* out = (float*)carve(elems * 4);
    int* labels = (int*)carve(elems * 4);
    void* scratch = carve(need);
    int* nles = (int*)carve((size_t)C * 4);
    int* top = (int*)carve((size_t)C * 32 * 8 * 4);
    int* profile = (int*)carve((size_t)C * 32 * N * 4);
    void* st = (void*)(uintptr_t)0x5000;
    for (int across = 0; across < 2; ++across) {
      if (octseg_volume_components(a, N, H, W, C, across, scratch, need, labels, nles, top, profile, st) != 0) {
        fprintf(stderr, "volume_components: %s\n", octseg_last_error());
        return 41;
      }
      if (octseg_volume_components(a, N, H, W, C, across, scratch, need, labels, nullptr, nullptr, nullptr, st) != 0) return 41;
      if (octseg_volume_components(a, N, H, W, C, across, scratch, need, nullptr, nullptr, nullptr, profile, st) != 0) return 41;
      if (octseg_volume_cleanup(a, N, H, W, C, across, 3, 2, 2, scratch, need, out, nles, top, st) != 0) {
        fprintf(stderr, "volume_cleanup: %s\n", octseg_last_error());
        return 42;
      }
      if (octseg_volume_cleanup(a, N, H, W, C, across, 0, 0, 1, scratch, need, out, nullptr, nullptr, st) != 0) return 42;
    }
    // refused before anything is enqueued
    const unsigned long long before = dry_launches() + dry_memops();
    if (octseg_volume_components(a, N, H, W, C, 0, scratch, need - 1, labels, nles, top, profile, st) == 0 ||
        octseg_volume_components(a, N, H, W, C, 2, scratch, need, labels, nles, top, profile, st) == 0 ||
        octseg_volume_components(a, N, H, W, 17, 0, scratch, need, labels, nles, top, profile, st) == 0 ||
        octseg_volume_components(a, N, H, W, C, 0, scratch, need, nullptr, nullptr, nullptr, nullptr, st) == 0 ||
        octseg_volume_components(a, N, H, W, C, 0, (char*)scratch + 4, need, labels, nles, top, profile, st) == 0 ||
        octseg_volume_cleanup(a, N, H, W, C, 0, 0, 0, 0, scratch, need, out, nles, top, st) == 0 ||
        octseg_volume_cleanup(a, N, H, W, C, 0, -1, 0, 2, scratch, need, out, nles, top, st) == 0 ||
        octseg_volume_cleanup(a, N, H, W, C, 0, 0, -1, 2, scratch, need, out, nles, top, st) == 0 ||
        octseg_volume_cleanup(a, N, H, W, C, 0, 0, 0, 2, scratch, need, a, nles, top, st) == 0 ||
        octseg_volume_cleanup(a, N, H, W, C, 0, 0, 0, 2, scratch, need, nullptr, nles, top, st) == 0)
      return 43;
    if (dry_launches() + dry_memops() != before) { fprintf(stderr, "a refused lesion call enqueued work\n"); return 44; }
  }
  if (octseg_lesions_scratch_bytes(1, 2048, 1024, 1024) != 0 || octseg_lesions_scratch_bytes(17, 2, 8, 8) != 0 || octseg_lesions_scratch_bytes(1, 0, 8, 8) != 0)
    return 45;
  return 0;
}

// The lesion-matching entry points (csrc/match.hip, csrc/match_api.cpp) against the stubs: the scratch carving of two labellings that share their
// counters, the memsets (overlap, frames, the lesion counter of either side) inside their ranges and every grid, from a single voxel to a volume
// just under 2^31 - 1 voxels, with and without the optional outputs and with one buffer on both sides; then what the call must refuse.
int exercise_match() {
  char* base = (char*)(uintptr_t)0x500000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  const int shapes[][4] = {{1, 1, 1, 1}, {5, 97, 130, 5}, {186, 704, 704, 4}, {2047, 1024, 1024, 16}};
  for (auto& sh : shapes) {
    dry_clear_ranges();
    const int N = sh[0], H = sh[1], W = sh[2], C = sh[3];
    const size_t need = octseg_match_scratch_bytes(C, N, H, W);
    if (need == 0 || need <= octseg_match_scratch_bytes(1, N, H, W) - (C == 1) || need <= octseg_lesions_scratch_bytes(C, N, H, W)) return 70;
    const size_t elems = (size_t)N * H * W * C;
    float* a = (float*)carve(elems * 4);
    float* b = (float*)carve(elems * 4);
    void* scratch = carve(need);
    int* nles = (int*)carve((size_t)C * 2 * 4);
    int* top = (int*)carve((size_t)C * 2 * 32 * 8 * 4);
    int* overlap = (int*)carve((size_t)C * 33 * 33 * 4);
    int* frames = (int*)carve((size_t)C * N * 3 * 4);
    void* st = (void*)(uintptr_t)0x5000;
    for (int across = 0; across < 2; ++across) {
      if (octseg_volume_match(a, b, N, H, W, C, across, scratch, need, nles, top, overlap, frames, st) != 0) {
        fprintf(stderr, "volume_match: %s\n", octseg_last_error());
        return 71;
      }
      if (octseg_volume_match(a, a, N, H, W, C, across, scratch, need, nles, nullptr, overlap, nullptr, st) != 0) return 71;
      if (octseg_volume_match(a, b, N, H, W, C, across, scratch, need, nles, top, overlap, nullptr, st) != 0) return 71;
      if (octseg_volume_match(a, b, N, H, W, C, across, scratch, need, nles, nullptr, overlap, frames, st) != 0) return 71;
    }
    // refused before anything is enqueued
    const unsigned long long before = dry_launches() + dry_memops();
    if (octseg_volume_match(nullptr, b, N, H, W, C, 0, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, nullptr, N, H, W, C, 0, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 0, nullptr, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 0, scratch, need, nullptr, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 0, scratch, need, nles, top, nullptr, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 0, scratch, need - 1, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 2, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, 17, 0, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, 0, 0, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, 0, H, W, C, 0, scratch, need, nles, top, overlap, frames, st) == 0 ||
        octseg_volume_match(a, b, N, H, W, C, 0, (char*)scratch + 4, need, nles, top, overlap, frames, st) == 0)
      return 72;
    if (dry_launches() + dry_memops() != before) { fprintf(stderr, "a refused match call enqueued work\n"); return 73; }
  }
  if (octseg_volume_match((float*)8, (float*)8, 2048, 1024, 1024, 1, 0, (void*)8, (size_t)1 << 60, (int*)8, nullptr, (int*)8, nullptr, nullptr) == 0) return 74;
  if (octseg_match_scratch_bytes(1, 2048, 1024, 1024) != 0 || octseg_match_scratch_bytes(17, 2, 8, 8) != 0 || octseg_match_scratch_bytes(1, 0, 8, 8) != 0)
    return 75;
  return 0;
}

// The mask clean-up entry points (csrc/components.hip over the shared kernels of csrc/bitplanes.hip, csrc/api.cpp) against the stubs: the scratch
// carving, the memset of the component counters inside its range and every grid, from a single pixel to a frame just under 2^31 - 1 pixels;
// every combination of outputs and of the smoothing, the filter and the fill; then what they must refuse.
int exercise_components() {
  char* base = (char*)(uintptr_t)0x400000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 97, 130, 5}, {186, 1000, 1000, 4}, {1, 46340, 46340, 1}};      // 46340^2 = 2^31 - 88048
  for (auto& sh : shapes) {
    dry_clear_ranges();
    const int N = sh[0], H = sh[1], W = sh[2], C = sh[3];
    const size_t need = octseg_components_scratch_bytes(N * C, H, W);
    if (need == 0 || need <= octseg_components_scratch_bytes(1, H, W) - (N * C == 1)) return 50;
    const size_t elems = (size_t)N * H * W * C;
    float* a = (float*)carve(elems * 4);
    float* out = (float*)carve(elems * 4);
    int* labels = (int*)carve(elems * 4);
    void* scratch = carve(need);
    int* ncomp = (int*)carve((size_t)N * C * 4);
    int* top = (int*)carve((size_t)N * C * 8 * 6 * 4);
    void* st = (void*)(uintptr_t)0x5000;
    for (int mask = 1; mask < 8; ++mask)            // labels, ncomp, top: each combination that asks for something
      if (octseg_stack_components(a, N, H, W, C, scratch, need, mask & 1 ? labels : nullptr, mask & 2 ? ncomp : nullptr, mask & 4 ? top : nullptr, st) != 0) {
        fprintf(stderr, "stack_components: %s\n", octseg_last_error());
        return 51;
      }
    for (int smooth_k : {0, 1, 2, 7})
      for (int filter = 0; filter < 3; ++filter)    // no filter, keep-largest, min_area
        for (int fill = 0; fill < 2; ++fill)
          for (int tables = 0; tables < 2; ++tables)
            if (octseg_stack_cleanup(a, N, H, W, C, smooth_k, filter == 1 ? 3 : 0, filter == 2 ? 5 : 0, fill, scratch, need, out, tables ? ncomp : nullptr,
                                     tables ? top : nullptr, st) != 0) {
              fprintf(stderr, "stack_cleanup: %s\n", octseg_last_error());
              return 52;
            }
    // refused before anything is enqueued
    const unsigned long long before = dry_launches() + dry_memops();
    if (octseg_stack_components(a, N, H, W, C, scratch, need - 1, labels, ncomp, top, st) == 0 ||
        octseg_stack_components(a, N, H, W, C, nullptr, need, labels, ncomp, top, st) == 0 ||
        octseg_stack_components(a, N, H, W, C, (char*)scratch + 4, need, labels, ncomp, top, st) == 0 ||
        octseg_stack_components(a, N, H, W, 17, scratch, need, labels, ncomp, top, st) == 0 ||
        octseg_stack_components(a, N, 0, W, C, scratch, need, labels, ncomp, top, st) == 0 ||
        octseg_stack_components(a, N, H, W, C, scratch, need, nullptr, nullptr, nullptr, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 8, 3, 0, 1, scratch, need, out, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, -1, 3, 0, 1, scratch, need, out, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 2, -1, 0, 1, scratch, need, out, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 2, 3, -1, 1, scratch, need, out, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 2, 3, 0, 1, scratch, need - 1, out, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 2, 3, 0, 1, scratch, need, a, ncomp, top, st) == 0 ||
        octseg_stack_cleanup(a, N, H, W, C, 2, 3, 0, 1, scratch, need, nullptr, ncomp, top, st) == 0)
      return 53;
    if (dry_launches() + dry_memops() != before) { fprintf(stderr, "a refused clean-up call enqueued work\n"); return 54; }
  }
  if (octseg_components_scratch_bytes(1, 46341, 46341) != 0 || octseg_components_scratch_bytes(0, 8, 8) != 0 || octseg_components_scratch_bytes(1, 8, 0) != 0)
    return 55;
  return 0;
}
// The contour entry points (csrc/contours.hip, csrc/contours_api.cpp) against the stubs: the scratch carving with its per-edge arrays, the memset of
// the counts inside its range and every grid (the scans' tile counts, the jump rounds) from a single pixel to the largest frame an edge id allows
// and to the largest capacity; then what they must refuse.
int exercise_contours() {
  char* base = (char*)(uintptr_t)0x500000000000ull;
  auto carve = [&](size_t bytes) { char* r = base; base += (bytes + 4095) / 4096 * 4096 + 4096; dry_register_range(r, bytes); return r; };
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 97, 130, 5}, {186, 704, 704, 4}, {1, 23169, 23169, 1}, {2, 64, 1 << 22, 16}};      // 23170^2 < 2^29
  const long long caps[] = {1, 4, 100000, (1ll << 31) - 1};
  for (auto& sh : shapes) {
    const int N = sh[0], H = sh[1], W = sh[2], C = sh[3];
    for (long long ecap : caps) {
      dry_clear_ranges();
      const size_t need = octseg_contours_scratch_bytes(N * C, H, W, ecap);
      if (need == 0 || need <= octseg_contours_scratch_bytes(1, H, W, ecap) - (N * C == 1)) return 60;
      if (ecap > 1 && (need < octseg_contours_scratch_bytes(N * C, H, W, ecap - 1) || (ecap >= 100000 && need <= octseg_contours_scratch_bytes(N * C, H, W, 1))))
        return 62;                                  // grows with the capacity (in 256-byte steps)
      float* a = (float*)carve((size_t)N * H * W * C * 4);
      void* scratch = carve(need);
      long long* counts = (long long*)carve((size_t)N * C * 2 * 8);
      int* ncont = (int*)carve((size_t)N * C * 4);
      int* table = (int*)carve((size_t)OCTSEG_CONTOUR_FIELDS * 4 * 16);
      int* verts = (int*)carve(2 * 4 * 16);
      int* overflow = (int*)carve(4);
      void* st = (void*)(uintptr_t)0x5000;
      if (octseg_stack_contour_counts(a, N, H, W, C, counts, st) != 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 16, ncont, table, verts, overflow, st) != 0) {
        fprintf(stderr, "contours: %s\n", octseg_last_error());
        return 61;
      }
      // refused before anything is enqueued
      const unsigned long long before = dry_launches() + dry_memops();
      if (octseg_stack_contour_counts(nullptr, N, H, W, C, counts, st) == 0 || octseg_stack_contour_counts(a, N, H, W, C, nullptr, st) == 0 ||
          octseg_stack_contour_counts(a, N, H, W, C, (long long*)((char*)counts + 4), st) == 0 ||
          octseg_stack_contour_counts(a, N, H, W, 17, counts, st) == 0 || octseg_stack_contour_counts(a, 0, H, W, C, counts, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need - 1, ecap, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, nullptr, need, ecap, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, (char*)scratch + 4, need, ecap, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, 17, scratch, need, ecap, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, 0, W, C, scratch, need, ecap, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, 0, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, 1ll << 31, 16, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 0, 16, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 1ll << 31, ncont, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 16, nullptr, table, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 16, ncont, nullptr, verts, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 16, ncont, table, nullptr, overflow, st) == 0 ||
          octseg_stack_contours(a, N, H, W, C, scratch, need, ecap, 16, 16, ncont, table, verts, nullptr, st) == 0)
        return 63;
      if (dry_launches() + dry_memops() != before) { fprintf(stderr, "a refused contour call enqueued work\n"); return 64; }
    }
  }
  // an edge id must fit 31 bits; H * W below 2^31 - 1; the vertex words of a call below 2^31
  if (octseg_contours_scratch_bytes(1, 23170, 23170, 8) != 0 || octseg_contours_scratch_bytes(1, 46341, 46341, 8) != 0 ||
      octseg_contours_scratch_bytes(0, 8, 8, 8) != 0 || octseg_contours_scratch_bytes(1, 8, 0, 8) != 0 || octseg_contours_scratch_bytes(1, 8, 8, 0) != 0 ||
      octseg_contours_scratch_bytes(1, 8, 8, 1ll << 31) != 0 || octseg_contours_scratch_bytes(1 << 30, 4, 4, 8) != 0)
    return 65;
  return 0;
}
}  // namespace

int main() {
  const char* archs[] = {"unet", "unetplusplus", "linknet", "fpn", "deeplabv3plus", "pspnet", "deeplabv3", "manet", "pan"};
  const char* encs[] = {"resnet18", "resnet34", "resnet50", "resnet101", "resnet152", "timm-regnetx_002", "timm-regnetx_064", "timm-regnety_120",
                        "efficientnet-b0", "efficientnet-b5", "efficientnet-b7"};
  const int shapes[][3] = {{1, 32, 32}, {16, 704, 704}, {3, 96, 64}, {2, 64, 160}};      // (PAN needs >= 128 x 128 to run: its frames are doubled below)
  int plans = 0, executed = 0;
  unsigned long long checksum = 0;
  for (const char* arch : archs)
    for (const char* enc : encs)
      for (auto& sh : shapes)
        for (int dtype = 0; dtype < 3; ++dtype)
          for (int classes : {1, 4}) {
            if (classes == 4 && !(sh[1] == 96 || dtype == 1)) continue;   // (the class count only changes the head: a subset is enough)
            // Encoders outside the ResNets (timm RegNet: grouped convs as per-group layers on channel slices; EfficientNet: MBConv blocks):
            // built under U-Net, U-Net++ and FPN always; LinkNet / PSPNet only where a QUARTER of the feature widths is a multiple of the
            // 8-channel vector (RegNetY-120 both, EfficientNet-B5 PSPNet); the dilated DeepLab encoders never.  The builder refuses the rest
            // with OCTSEG_UNSUPPORTED_ARCH (checked here for every refused pair).
            const bool other_enc = !strncmp(enc, "timm-", 5) || !strncmp(enc, "efficientnet-", 13);
            if (other_enc && !strcmp(arch, "pan")) {        // PAN dilates its encoder: ResNets only
              octseg_net_desc dr{arch, enc, classes, sh[0], sh[1], sh[2], dtype};
              octseg_plan* pr = nullptr;
              if (octseg_plan_create(&dr, &pr) != OCTSEG_UNSUPPORTED_ARCH || pr) { fprintf(stderr, "pan over %s was not refused\n", enc); return 7; }
              continue;
            }
            if (other_enc && (!strcmp(arch, "linknet") || !strcmp(arch, "pspnet") || !strncmp(arch, "deeplab", 7))) {
              const bool ok_pair = (!strcmp(enc, "timm-regnety_120") && strncmp(arch, "deeplab", 7)) || (!strcmp(enc, "efficientnet-b5") && !strcmp(arch, "pspnet"));
              if (!ok_pair) {
                octseg_net_desc dr{arch, enc, classes, sh[0], sh[1], sh[2], dtype};
                octseg_plan* pr = nullptr;
                if (octseg_plan_create(&dr, &pr) != OCTSEG_UNSUPPORTED_ARCH || pr) { fprintf(stderr, "%s over %s was not refused\n", arch, enc); return 7; }
                continue;
              }
            }
            const int fs = (!strcmp(arch, "pan") && sh[1] < 128) ? 2 : 1;
            octseg_net_desc d{arch, enc, classes, sh[0], sh[1] * fs, sh[2] * fs, dtype};
            octseg_plan* p = nullptr;
            if (octseg_plan_create(&d, &p) != 0 || !p) {
              fprintf(stderr, "plan_create(%s, %s, B=%d %dx%d, dtype %d) failed: %s\n", arch, enc, sh[0], sh[1], sh[2], dtype, octseg_last_error());
              return 2;
            }
            ++plans;
            const size_t ws = octseg_plan_workspace_bytes(p), np = octseg_plan_param_numel(p), nb = octseg_plan_buffer_numel(p);
            checksum += ws % 1000003 + np + nb;
            size_t covered = 0;
            std::string first_conv;
            for (int i = 0; i < octseg_plan_num_params(p); ++i) {
              octseg_param_info pi;
              if (octseg_plan_param_info(p, i, &pi) != 0) return 3;
              if (pi.offset + pi.numel > np) { fprintf(stderr, "%s: parameter %s leaves the arena\n", arch, pi.name); return 4; }
              if (pi.offset < covered) { fprintf(stderr, "%s: parameter %s overlaps its predecessor\n", arch, pi.name); return 4; }
              covered = pi.offset + pi.numel;
              const size_t n = strlen(pi.name);
              if (first_conv.empty() && pi.kind == OCTSEG_P_CONV && n > 7 && strcmp(pi.name + n - 7, ".weight") == 0)
                first_conv.assign(pi.name, n - 7);
            }
            for (int i = 0; i < octseg_plan_num_bn(p); ++i) {
              octseg_bn_info bi;
              if (octseg_plan_bn_info(p, i, &bi) != 0) return 3;
              if (bi.mean_offset + bi.C > nb || bi.var_offset + bi.C > nb) { fprintf(stderr, "BN %s leaves the buffer arena\n", bi.name); return 4; }
            }
            size_t ao = 0, go = 0; int dims[4] = {0, 0, 0, 0};
            if (!first_conv.empty() && octseg_plan_find_tensor(p, first_conv.c_str(), &ao, &go, dims) == 0) {
              const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * dims[3] * (dtype == 0 ? 4 : 2);
              if (ao + bytes > ws || go + bytes > ws) { fprintf(stderr, "%s: tensor of %s leaves the workspace\n", arch, first_conv.c_str()); return 4; }
            }
            if (octseg_plan_fwd_macs(p) <= 0) return 5;
            // error paths: out-of-range queries must fail cleanly
            octseg_param_info bad;
            if (octseg_plan_param_info(p, -1, &bad) == 0 || octseg_plan_param_info(p, octseg_plan_num_params(p), &bad) == 0) return 6;
            if (octseg_plan_find_tensor(p, "no.such.layer", nullptr, nullptr, nullptr) == 0) return 6;
            octseg_plan_params_changed(p);
            // the executors: every pair on the small non-square frame (all dtypes), the three BASELINE training configs at full size
            const bool base_cfg = sh[1] == 704 && dtype == 1 && classes == 1 &&
                                  ((!strcmp(arch, "unetplusplus") && !strcmp(enc, "resnet101")) || (!strcmp(arch, "linknet") && !strcmp(enc, "resnet50")) ||
                                   (!strcmp(arch, "unet") && !strcmp(enc, "resnet50")));
            if (sh[1] == 64 || base_cfg || (sh[1] == 96 && classes == 4)) {
              const int rc = exercise(d, p);
              if (rc) { fprintf(stderr, "exercise(%s, %s, B=%d %dx%d, dtype %d) -> %d\n", arch, enc, sh[0], sh[1], sh[2], dtype, rc); return rc; }
              ++executed;
            }
            octseg_plan_destroy(p);
          }
  // shapes the builder must refuse (smp check_input_shape / argument checks) without touching memory it does not own
  octseg_plan* q = nullptr;
  octseg_net_desc badr1{"linknet", "timm-regnetx_002", 1, 1, 32, 32, 0}, badr2{"deeplabv3plus", "timm-regnetx_064", 1, 2, 64, 64, 1},
      badr3{"pspnet", "timm-regnetx_002", 1, 2, 64, 64, 0};
  if (octseg_plan_create(&badr1, &q) == 0 || octseg_plan_create(&badr2, &q) == 0 || octseg_plan_create(&badr3, &q) == 0) { fprintf(stderr, "an unsupported RegNet pair was accepted\n"); return 7; }
  octseg_net_desc bad1{"unet", "resnet18", 1, 1, 48, 64, 0}, bad2{"segformer", "resnet18", 1, 1, 32, 32, 0}, bad3{"unet", "vgg", 1, 1, 32, 32, 0},
      bad4{"unet", "resnet18", 0, 1, 32, 32, 0}, bad5{"unet", "resnet18", 1, 1, 32, 32, 7};
  for (octseg_net_desc* b : {&bad1, &bad2, &bad3, &bad4, &bad5})
    if (octseg_plan_create(b, &q) == 0) { fprintf(stderr, "a bad descriptor was accepted\n"); return 7; }
  for (int dt = 0; dt < 3; ++dt) checksum += octseg_conv2d_scratch_bytes(dt, 2, 64, 64, 24, 40, 3, 3) + octseg_conv2d_scratch_bytes(dt, 1, 8, 8, 2048, 512, 1, 1);
  if (const int rc = exercise_distance()) { fprintf(stderr, "exercise_distance -> %d\n", rc); return rc; }
  if (const int rc = exercise_lesions()) { fprintf(stderr, "exercise_lesions -> %d\n", rc); return rc; }
  if (const int rc = exercise_match()) { fprintf(stderr, "exercise_match -> %d\n", rc); return rc; }
  if (const int rc = exercise_components()) { fprintf(stderr, "exercise_components -> %d\n", rc); return rc; }
  if (const int rc = exercise_contours()) { fprintf(stderr, "exercise_contours -> %d\n", rc); return rc; }
  if (dry_errors() != 0) { fprintf(stderr, "%llu launch / memory-range violations\n", dry_errors()); return 8; }
  printf("plan_dryrun: %d plans built, %d of them run through forward / backward / optimizer with recording HIP stubs (%llu launches, %llu memory "
         "operations checked) under ASan + UBSan, checksum %llu, 0 errors, launch fingerprint %016llx\n", plans, executed, dry_launches(), dry_memops(), checksum,
         dry_fingerprint());
  return 0;
}
