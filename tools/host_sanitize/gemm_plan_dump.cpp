// Host-only dump of the GEMM dispatch decision (csrc/gemm_plan.cpp, which holds no kernel: this builds in seconds and needs no GPU).
// Reads a list of GemmArgs descriptors (tests/gemm_dispatch_cases.txt: key=value per line, '#' comments) and prints one line each:
//   family bn splitk gn_rows ln_tiles fused_qkv_ok halo_width
// fused_qkv_ok: what the UNet's q | k | V^T site asks (vt_out set and the weight-stationary kernel); halo_width: conv3x3_halo_width().
// --stable: instead, print every descriptor whose plan changes once gn_part / ln_part are set from it (none may).
// tests/test_gemm_plan_cpu.py compares the output with the tables recorded from the dispatch code this plan replaced.
#include "kernels.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace SDNS;

// the library's cached lookup lives in runtime.cpp beside the context: here a plain read of the environment
int64_t svg_env_i64(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return (e && *e) ? atoll(e) : dflt;
}

static char dummy[64];      // what a set pointer field points at (never read)

static bool parse(const char* line, GemmArgs& g) {
  g = GemmArgs();
  char buf[1024];
  snprintf(buf, sizeof(buf), "%s", line);
  int n = 0;
  for (char* tok = strtok(buf, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
    if (tok[0] == '#') break;
    char* eq = strchr(tok, '=');
    if (!eq) { fprintf(stderr, "bad token '%s'\n", tok); exit(2); }
    *eq = 0;
    const long long v = atoll(eq + 1);
    const std::string k = tok;
    ++n;
    if (k == "M") g.M = (int)v; else if (k == "N") g.N = (int)v; else if (k == "K") g.K = (int)v;
    else if (k == "amode") g.amode = (int)v; else if (k == "H") g.H = (int)v; else if (k == "W") g.W = (int)v; else if (k == "Cin") g.Cin = (int)v;
    else if (k == "Ho") g.Ho = (int)v; else if (k == "Wo") g.Wo = (int)v; else if (k == "batch") g.batch = (int)v;
    else if (k == "lda") g.lda = (int)v; else if (k == "ldb") g.ldb = (int)v; else if (k == "ldc") g.ldc = (int)v; else if (k == "ldr") g.ldr = (int)v;
    else if (k == "n_valid") g.n_valid = (int)v; else if (k == "act") g.act = (int)v; else if (k == "out_f32") g.out_f32 = (int)v;
    else if (k == "bias_row") g.bias_row = (int)v; else if (k == "bias_bn") g.bias_bn = v ? (const float*)dummy : nullptr;
    else if (k == "ln_rs") g.ln_rs = g.ln_rm = g.ln_s = v ? (const float*)dummy : nullptr; else if (k == "ln_swapped") g.ln_swapped = (int)v;
    else if (k == "A2") g.A2 = v ? (const h16*)dummy : nullptr; else if (k == "lda2") g.lda2 = (int)v; else if (k == "k_split") g.k_split = (int)v;
    else if (k == "residual") g.residual = v ? (const h16*)dummy : nullptr;
    else if (k == "vt_out") g.vt_out = v ? (h16*)dummy : nullptr; else if (k == "vt_n0") g.vt_n0 = (int)v; else if (k == "vt_rows") g.vt_rows = (int)v;
    else if (k == "vt_ld") g.vt_ld = (int)v; else if (k == "gn_part") g.gn_part = v ? (float*)dummy : nullptr;
    else if (k == "ln_part") g.ln_part = v ? (float*)dummy : nullptr;
    else { fprintf(stderr, "unknown key '%s'\n", tok); exit(2); }
  }
  return n > 0;
}

int main(int argc, char** argv) {
  bool stable = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) { if (!strcmp(argv[i], "--stable")) stable = true; else path = argv[i]; }
  FILE* f = path ? fopen(path, "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: gemm_plan_dump [--stable] CASES\n"); return 2; }
  char line[1024];
  while (fgets(line, sizeof(line), f)) {
    GemmArgs g;
    if (!parse(line, g)) continue;
    const GemmPlan p = gemm_plan(g);
    if (!stable) {
      printf("%d %d %d %d %d %d %d\n", p.family, p.bn, p.splitk, p.gn_rows, p.ln_tiles, g.vt_out && p.family == GF_WS ? 1 : 0, p.family == GF_HALO ? p.bn : 0);
      continue;
    }
    GemmArgs h = g;
    if (p.gn_rows > 0) h.gn_part = (float*)dummy;
    if (p.ln_tiles > 0) { h.ln_part = (float*)dummy; h.ln_tiles = p.ln_tiles; }
    const GemmPlan q = gemm_plan(h);
    if (!(p == q)) printf("UNSTABLE %d %d %d %d %d -> %d %d %d %d %d : %s", p.family, p.bn, p.splitk, p.gn_rows, p.ln_tiles, q.family, q.bn, q.splitk, q.gn_rows, q.ln_tiles, line);
  }
  fclose(f);
  return 0;
}
