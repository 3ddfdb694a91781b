// The weight-gradient launcher's host arithmetic under AddressSanitizer / UBSan, as a stand-alone program (no GPU, no Python):
// w2l_wgrad_launch_plan over the edge shapes and the forced sweeps of tests/golden/wgrad_plans.json (tools/record_wgrad_plans.py
// holds the same lists), w2l_wgrad_dealt_segments, and w2l_tune_load / w2l_tune_save on a temporary file.
//
//   cd wav2letter_pytorch_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       ../../tools/wgrad_plan_sanitize.cpp runtime.hip conv_wgrad.hip conv_wgrad_fp8.hip -o /tmp/wgrad_plan_sanitize && /tmp/wgrad_plan_sanitize
//
// The implicit GEMM's four tune-file functions and the three-tap code object are stubbed below, so that the launcher's sources
// link without the rest of the library.  Exit status 0 and "ok" on the last line: clean.
#include "../include/w2l_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

void w2l_igemm_tune_dump(FILE*) {}
bool w2l_igemm_tune_put(const int*) { return false; }
void w2l_igemm_fp8_tune_dump(FILE*) {}
bool w2l_igemm_fp8_tune_put(const int*) { return false; }
extern "C" const unsigned char w2l_wgrad3_hsaco[1] = {0};
extern "C" const unsigned int w2l_wgrad3_hsaco_len = 0;

static long g_launches = 0, g_refused = 0;

static void query(const int* sh, long long ws, int splits, int order) {
    int out[W2L_WGRAD_PLAN_FIELDS];
    const int rc = w2l_wgrad_launch_plan(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], ws, splits, order, out);
    if ((rc == 0) != (out[W2L_WGRAD_PLAN_FIELDS - 1] == 1)) { printf("inconsistent answer\n"); exit(1); }
    (rc == 0 ? g_launches : g_refused) += 1;
    (void)w2l_wgrad_needs_zero_x(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], ws);
    (void)w2l_wgrad_needs_zero(sh[0], sh[1], sh[2], sh[3], sh[4]);
    (void)w2l_wgrad_plan(sh[0], sh[1], sh[2], sh[3], sh[4]);
}

int main() {
    const int edges[][7] = {{2, 128, 128, 40, 5, 1, 1}, {1, 64, 64, 64, 3, 1, 1}, {1, 256, 256, 1, 11, 1, 1}, {4, 256, 384, 200, 1, 1, 1},
                            {4, 256, 384, 200, 2, 1, 1}, {4, 256, 384, 200, 3, 1, 1}, {4, 256, 384, 200, 7, 1, 4}, {4, 256, 384, 200, 7, 1, 5},
                            {16, 128, 256, 300, 9, 2, 1}, {16, 128, 256, 300, 3, 2, 3}, {16, 64, 64, 700, 5, 1, 1}, {2, 2048, 2048, 130, 9, 1, 1},
                            {2, 1024, 1024, 130, 31, 1, 1}, {4, 256, 256, 200, 3, 1, 200}, {4, 256, 256, 200, 3, 4, 40},
                            {0, 64, 64, 10, 3, 1, 1}, {1, 100, 64, 10, 3, 1, 1}, {1, 64, 64, 10, 0, 1, 1}};
    const int sweeps[][7] = {{3, 192, 320, 335, 7, 1, 1}, {8, 64, 256, 500, 11, 2, 1}, {32, 896, 896, 500, 29, 1, 2}};
    const int counts[] = {1, 2, 3, 5, 18, 32, 40, 97, 256, 512, 1024, 1025};
    auto workspaces = [](const int* sh, long long* ws) {
        const long long a = w2l_wgrad_workspace_bytes(sh[1], sh[2], sh[4]), b = w2l_wgrad_dealt_workspace_bytes(sh[1], sh[2], sh[4]);
        ws[0] = 0; ws[1] = 65536; ws[2] = a; ws[3] = b; ws[4] = a > b ? a : b;
    };
    for (int det = 0; det < 2; ++det) {
        w2l_wgrad_deterministic(det);
        for (const auto& sh : edges) {
            long long ws[5];
            workspaces(sh, ws);
            for (long long w : ws) query(sh, w, 0, -1);
        }
    }
    w2l_wgrad_deterministic(0);
    for (const auto& sh : sweeps) {
        long long ws[5];
        workspaces(sh, ws);
        for (int order = 0; order < 128; ++order)
            for (int s : counts)
                for (long long w : {0LL, ws[4]}) {
                    query(sh, w, s, order);
                    w2l_wgrad_force_plan(s, order);          // and once through the per-thread hook
                    query(sh, w, 0, -1);
                    w2l_wgrad_force_plan(0, -1);
                }
    }
    // dealt segments: geometries with and without a dealt form, and an output buffer shorter than the block count
    const int geo[][3] = {{175, 256, 512}, {1, 24, 7}, {18, 18, 97}, {1024, 60, 1024}, {513, 256, 512}, {7, 3, 8}, {3, 1, 1025}};
    for (const auto& g : geo) {
        std::vector<int> buf(6 * 2 * g[2]);
        const int n = w2l_wgrad_dealt_segments(g[0], g[1], g[2], buf.data(), 2 * g[2]);
        std::vector<int> small(6 * 3);
        const int m = w2l_wgrad_dealt_segments(g[0], g[1], g[2], small.data(), 3);
        if (n != m || n > 2 * g[2]) { printf("dealt segments: %d / %d blocks\n", n, m); return 1; }
    }
    // the tune file: load plans (and lines that are not), see them take effect, save them, load the saved file again
    char path[] = "/tmp/w2l_wgrad_tune_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { printf("mkstemp failed\n"); return 1; }
    FILE* f = fdopen(fd, "w");
    fputs("w2l-tune v2 gfx950\nwgrad 7 256 256 500 11 512 33\nwgrad 7 384 384 500 13 1 3\nwgrad 7 512 512 500 17 4 65\n"
          "wgrad 7 896 896 500 29 3 17\nwgrad 7 640 640 500 21 2 21\nwgrad 7 64 64 500 3 9999 1\nwgrad 7 64 64 500 3 4 24\n"
          "wgradf8 7 256 256 500 11 4 1\nwgrad 1 2 3\n", f);
    fclose(f);
    const int taken = w2l_tune_load(path);
    const int cached[][7] = {{7, 256, 256, 500, 11, 1, 1}, {7, 384, 384, 500, 13, 1, 1}, {7, 512, 512, 500, 17, 1, 1}, {7, 896, 896, 500, 29, 1, 5},
                             {7, 896, 896, 500, 29, 2, 1}, {7, 640, 640, 500, 21, 1, 4}};
    for (const auto& sh : cached) {
        long long ws[5];
        workspaces(sh, ws);
        for (long long w : ws) query(sh, w, 0, -1);
    }
    const bool dealt = w2l_wgrad_plan(7, 256, 256, 500, 11) == (33 | (512 << 8));
    const int saved = w2l_tune_save(path), again = w2l_tune_load(path);
    remove(path);
    if (taken != 6 || !dealt || saved != 0 || again != 6) { printf("tune file: %d taken, %d saved, %d again\n", taken, saved, again); return 1; }
    if (w2l_tune_load("/nonexistent/w2l_tune") != -1) return 1;
    printf("%ld launches planned, %ld refused\nok\n", g_launches, g_refused);
    return 0;
}
