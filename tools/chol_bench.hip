// Correctness + timing of the device Cholesky solves (developer tool, not part of the product):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I go_slam_amd/csrc -o /tmp/chol_bench tools/chol_bench.hip && /tmp/chol_bench 150 294 ...
// For every n: max residual |(A + D) x - b| of the product's dispatch (chol_small_kernel for n <= 192, chol_mid_kernel up
// to MID_N, the blocked path above) and of the blocked path forced through gs_chol_solve's `path`, their agreement, and
// event-timed microseconds per solve; the phase stamps of chol_step_kernel (n > 450), chol_small_kernel (n <= 192) and
// chol_mid_kernel (192 < n <= 312); an indefinite system's dx and failure flag on both paths.
#define CHOL_TIMING 1
#include "../go_slam_amd/csrc/chol.hip"
#include <cstdio>
#include <vector>
#include <cmath>
void gs_set_error(const char* fmt, ...) {}
thread_local int gs_timing_on = 0;
void gs_timing_mark(const char*) {}

static double residual(const std::vector<double>& A, const std::vector<double>& b, const std::vector<float>& x, int n) {
  double worst = 0;
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int j = 0; j < n; ++j) { double a = A[(size_t)i * n + j]; if (i == j) a = a + (0.1 + 1e-4 * a); s += a * x[j]; }
    worst = fmax(worst, fabs(s - b[i]));
  }
  return worst;
}

int main(int argc, char** argv) {
  for (int ai = 1; ai < (argc > 1 ? argc : 2); ++ai) {
    const int n = argc > 1 ? atoi(argv[ai]) : 150;
    std::vector<double> A((size_t)n * n), b(n), M((size_t)n * n);
    srand(1);
    for (auto& v : M) v = (rand() / (double)RAND_MAX) - 0.5;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
      double s = 0; for (int k = 0; k < n; ++k) s += M[(size_t)i * n + k] * M[(size_t)j * n + k];
      A[(size_t)i * n + j] = s + (i == j ? n : 0);
    }
    for (int i = 0; i < n; ++i) b[i] = i * 0.01 - 0.3;
    double *dA, *db; float* dx; int32_t* flags;
    hipMalloc(&dA, A.size() * 8); hipMalloc(&db, n * 8); hipMalloc(&dx, n * 4); hipMalloc(&flags, 64);
    hipMemset(flags, 0, 64);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    // one solve of `mat` by `path` (CHOL_PATH_DISPATCH or CHOL_PATH_BLOCKED); returns its event-timed milliseconds
    auto solve = [&](const std::vector<double>& mat, int path) {
      hipMemcpy(dA, mat.data(), mat.size() * 8, hipMemcpyHostToDevice);
      hipMemcpy(db, b.data(), n * 8, hipMemcpyHostToDevice);
      hipDeviceSynchronize();
      hipEventRecord(e0);
      gs_chol_solve(dA, db, n, 1e-4f, 0.1f, path, dx, flags, 0);
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      return ms;
    };
    const int paths[2] = {CHOL_PATH_DISPATCH, CHOL_PATH_BLOCKED};
    std::vector<float> xs[2];
    float us[2] = {0, 0};
    for (int m = 0; m < 2; ++m) {
      float best = 1e9f;
      for (int rep = 0; rep < 6; ++rep) {
        const float ms = solve(A, paths[m]);
        if (rep > 0 && ms < best) best = ms;
      }
      us[m] = best * 1e3f;
      xs[m].resize(n);
      hipMemcpy(xs[m].data(), dx, n * 4, hipMemcpyDeviceToHost);
    }
    int32_t fl[2]; hipMemcpy(fl, flags, 8, hipMemcpyDeviceToHost);
    double dmax = 0, xmax = 0;
    for (int i = 0; i < n; ++i) { dmax = fmax(dmax, fabs((double)xs[0][i] - xs[1][i])); xmax = fmax(xmax, fabs((double)xs[0][i])); }
    printf("n %4d: product dispatch %7.1f us (residual %.3e) | multi-kernel %7.1f us (residual %.3e) | max |x - x_multi| %.3e of %.3e, fail flag %d count %d\n",
           n, us[0], residual(A, b, xs[0], n), us[1], residual(A, b, xs[1], n), dmax, xmax, fl[0], fl[1]);
    if (n > 450) {                                    // where the step kernel's panel wave spends a step (workgroup 0)
      long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      hipMemcpyToSymbol(HIP_SYMBOL(g_step_t), z, sizeof(z));
      solve(A, CHOL_PATH_BLOCKED);
      hipMemcpyFromSymbol(z, HIP_SYMBOL(g_step_t), sizeof(z));
      const double steps = (n - 1) / 32;
      printf("        chol_step panel wave, us per step: loads + staging %.2f | pending updates %.2f | diagonal factor %.2f | row solve %.2f | stores issued %.2f\n",
             z[0] / 100.0 / steps, z[1] / 100.0 / steps, z[2] / 100.0 / steps, z[3] / 100.0 / steps, z[4] / 100.0 / steps);
    }
    if (n <= 312) {
      solve(A, CHOL_PATH_DISPATCH);
      long long t[64];
      hipMemcpyFromSymbol(t, HIP_SYMBOL(g_chol_t), sizeof(t));
      auto usf = [&](int a, int c) { return (t[c] - t[a]) / 100.0; };
      if (n <= 192) {
        printf("        chol_small phases: load %.1f  factor %.1f  backward %.1f  total %.1f us; thread 0: diag %.1f rows %.1f panelupd %.1f barrier %.1f far %.1f\n",
               usf(0, 1), usf(1, 2), usf(2, 3), usf(0, 3), t[10] / 100.0, t[11] / 100.0, t[12] / 100.0, t[13] / 100.0, t[14] / 100.0);
      } else {
        printf("        chol_mid phases:");
        int prev = 20;
        for (int sgi = 0; sgi < 4 && t[21 + 4 * sgi] > t[20]; ++sgi) {
          const int q = 21 + 4 * sgi;
          printf(" stage %d: load %.1f factor %.1f global-update %.1f write-back %.1f |", sgi, usf(prev, q), usf(q, q + 1), usf(q + 1, q + 2), usf(q + 2, q + 3));
          prev = q + 3;
        }
        printf(" tail: load %.1f factor %.1f backward %.1f | heads: L21^T x %.1f stages %.1f | total %.1f us\n", usf(prev, 40), usf(40, 41), usf(41, 42), usf(42, 43), usf(43, 44), usf(20, 44));
      }
    }
    // an indefinite matrix must give dx = 0 and raise the flag on both paths
    std::vector<double> Aneg = A;
    Aneg[(size_t)(n / 2) * n + n / 2] = -1e6;
    for (int m = 0; m < 2; ++m) {
      solve(Aneg, paths[m]);
      std::vector<float> x(n); hipMemcpy(x.data(), dx, n * 4, hipMemcpyDeviceToHost);
      hipMemcpy(fl, flags, 8, hipMemcpyDeviceToHost);
      double nz = 0; for (float v : x) nz = fmax(nz, fabs((double)v));
      printf("        indefinite (%s): max |dx| %.1e, fail flag %d\n", m == 0 ? "product dispatch" : "multi-kernel", nz, fl[0]);
    }
    hipFree(dA); hipFree(db); hipFree(dx); hipFree(flags);
  }
  return 0;
}
