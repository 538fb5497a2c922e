// How long does a one-workgroup k_chain_potrf launch take while ANOTHER stream keeps every CU full
// of update workgroups?  Two streams in one process, created like the engine's (engine.cpp
// stream set): background = bulk (non-blocking, lowest priority), foreground = chain
// (non-blocking, highest priority).
//   background: ~150 ms of load (clocks, as update_bench.hip), then ONE saturating launch of, in
//     turn, k_update<64,16,2,2>, k_update<32,32,2,2>, k_update_dma128 on a synthetic DIRECT unit
//     (M = N = 8192, K = 512).  One pass over the unit takes ~1.1 ms, a train of 32 POTRF launches
//     beside it up to 2 ms, so the launch's tile list walks the unit kRepeat times: still one
//     launch, whose pending workgroups do not run out while the train is timed (checked: the
//     line says whether the train ended before the launch did).
//   foreground: a train of 32 k_chain_potrf launches of one 64 x 64 unit each (32 different SPD
//     blocks; the stream orders them), one event pair around the train.
// Prints us per POTRF launch alone and beside each background kernel (5 trains each: min / median).
// Build:
//   hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -I include -I spllt_amd/csrc scripts/placement_probe.hip -o placement_probe
#include "../spllt_amd/csrc/kernels.hip"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace spx;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  constexpr int M = 8192, N = 8192, K = 512, kTrain = 32, kRepeat = 6, kReps = 5, n = 64;
  int prio_lo = 0, prio_hi = 0;
  CK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  hipStream_t bg, fg;
  CK(hipStreamCreateWithPriority(&bg, hipStreamNonBlocking, prio_lo));
  CK(hipStreamCreateWithPriority(&fg, hipStreamNonBlocking, prio_hi));
  hipEvent_t warm, f0, f1, b0, b1;
  for (hipEvent_t* e : {&warm, &f0, &f1, &b0, &b1}) CK(hipEventCreate(e));

  // background unit (update_bench.hip)
  const int64_t src_elems = (int64_t)(M + N) * K, dst_elems = (int64_t)M * N;
  double* L;
  CK(hipMalloc(&L, (src_elems + dst_elems + 64) * 8));
  {
    std::vector<double> h(src_elems);
    for (int64_t i = 0; i < src_elems; ++i) h[i] = ((i * 2654435761u) % 1000) * 1e-3 - 0.5;
    CK(hipMemcpy(L, h.data(), src_elems * 8, hipMemcpyHostToDevice));
    CK(hipMemset(L + src_elems, 0, (dst_elems + 64) * 8));
  }
  int64_t bc_off_h[2] = {0, src_elems};
  int bc_w_h[2] = {K, N};
  int64_t* bc_off;
  int* bc_w;
  CK(hipMalloc(&bc_off, 16));
  CK(hipMalloc(&bc_w, 8));
  CK(hipMemcpy(bc_off, bc_off_h, 16, hipMemcpyHostToDevice));
  CK(hipMemcpy(bc_w, bc_w_h, 8, hipMemcpyHostToDevice));
  UpdUnit u{};
  u.d_off = src_elems; u.src_bcol0 = 0; u.nseg = 1; u.seg_r0 = 0; u.seg_stride = K;
  u.src_r0 = N; u.src_c0 = 0; u.M = M; u.N = N; u.k0 = 0; u.klen = -1; u.d_ld = N;
  u.d_row0 = 0; u.d_col0 = 0; u.mode = MODE_DIRECT; u.lower = 0; u.b_bcol0 = -1;
  u.a_off = 0; u.a_w = K;
  UpdUnit* du;
  CK(hipMalloc(&du, sizeof(u)));
  CK(hipMemcpy(du, &u, sizeof(u), hipMemcpyHostToDevice));

  // foreground: kTrain SPD blocks, one chain unit each
  std::vector<double> hA((size_t)kTrain * n * n);
  for (int b = 0; b < kTrain; ++b)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) hA[(size_t)b * n * n + i * n + j] = (i == j) ? n + 1.0 + b : 1.0 / (1 + abs(i - j));
  double *dA, *dinv;
  int* flag;
  CK(hipMalloc(&dA, hA.size() * 8));
  CK(hipMalloc(&dinv, hA.size() * 8));
  CK(hipMemset(dinv, 0, hA.size() * 8));
  CK(hipMalloc(&flag, 4));
  const int flag0 = INT_MAX;
  CK(hipMemcpy(flag, &flag0, 4, hipMemcpyHostToDevice));
  std::vector<ChainUnit> cu(kTrain);
  for (int b = 0; b < kTrain; ++b) {
    cu[b] = ChainUnit{};
    cu[b].off = (int64_t)b * n * n; cu[b].winv_off = (int64_t)b * n * n; cu[b].ld = n;
    cu[b].c0 = 0; cu[b].pn = n; cu[b].cs = 0; cu[b].ce = n; cu[b].gcol = b * n;
  }
  ChainUnit* dcu;
  CK(hipMalloc(&dcu, sizeof(ChainUnit) * kTrain));
  CK(hipMemcpy(dcu, cu.data(), sizeof(ChainUnit) * kTrain, hipMemcpyHostToDevice));

  auto train = [&]() {
    for (int b = 0; b < kTrain; ++b) launch_chain_panel(fg, dcu + b, 1, dA, dinv, flag, cu[b]);
  };
  const int tiles_of[4] = {0, 64, 32, 128};
  const char* names[4] = {"alone", "beside k_update<64,16,2,2>", "beside k_update<32,32,2,2>", "beside k_update_dma128"};
  for (int cfg = 0; cfg < 4; ++cfg) {
    const int T = tiles_of[cfg];
    const int Tw = T ? T : 128;   // "alone": the warm-up load still runs first (clocks)
    std::vector<UpdTile> tl;
    for (int rep = 0; rep < kRepeat; ++rep)
      for (int tj = 0; tj < N / Tw; ++tj)
        for (int ti = 0; ti < M / Tw; ++ti) tl.push_back(UpdTile{0, (short)ti, (short)tj});
    const int64_t pass = (int64_t)tl.size() / kRepeat;
    UpdTile* dt;
    CK(hipMalloc(&dt, tl.size() * sizeof(UpdTile)));
    CK(hipMemcpy(dt, tl.data(), tl.size() * sizeof(UpdTile), hipMemcpyHostToDevice));
    std::vector<float> us;
    float bg_ms = 0.f;
    int inside = 0;
    for (int r = 0; r < kReps; ++r) {
      CK(hipMemcpy(dA, hA.data(), hA.size() * 8, hipMemcpyHostToDevice));
      CK(hipDeviceSynchronize());
      for (int i = 0; i < 110; ++i) launch_update(bg, Tw, dt, pass, du, bc_off, bc_w, L, nullptr, nullptr, nullptr);
      CK(hipEventRecord(warm, bg));
      CK(hipEventRecord(b0, bg));
      if (T) launch_update(bg, T, dt, (int64_t)tl.size(), du, bc_off, bc_w, L, nullptr, nullptr, nullptr);
      CK(hipEventRecord(b1, bg));
      CK(hipStreamWaitEvent(fg, warm, 0));
      CK(hipEventRecord(f0, fg));
      train();
      CK(hipEventRecord(f1, fg));
      CK(hipDeviceSynchronize());
      float ms = 0.f, tail = 0.f;
      CK(hipEventElapsedTime(&ms, f0, f1));
      us.push_back(ms * 1e3f / kTrain);
      if (T) {
        CK(hipEventElapsedTime(&bg_ms, b0, b1));
        CK(hipEventElapsedTime(&tail, f1, b1));   // > 0: the train ended while the launch still ran
        inside += tail > 0.f;
      }
    }
    std::sort(us.begin(), us.end());
    if (T)
      printf("%-28s %6.1f us per POTRF launch (min), %6.1f (median); background launch %.2f ms, train inside it %d/%d\n",
             names[cfg], us.front(), us[us.size() / 2], bg_ms, inside, kReps);
    else
      printf("%-28s %6.1f us per POTRF launch (min), %6.1f (median)\n", names[cfg], us.front(), us[us.size() / 2]);
    fflush(stdout);
    CK(hipFree(dt));
  }
  int hflag = 0;
  CK(hipMemcpy(&hflag, flag, 4, hipMemcpyDeviceToHost));
  std::vector<double> Lh(n * n);
  CK(hipMemcpy(Lh.data(), dA, n * n * 8, hipMemcpyDeviceToHost));
  printf("check: flag %s, L[0][0] = %.6f (sqrt(65) = 8.062258)\n", hflag == INT_MAX ? "untouched" : "SET", Lh[0]);
  return hflag == INT_MAX ? 0 : 2;
}
