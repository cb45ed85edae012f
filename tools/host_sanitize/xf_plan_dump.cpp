// Host-only dump of the latent Transformer's forward plan and stage tables (csrc/xf_plan.cpp, which holds no kernel and makes no HIP
// call: this builds in seconds and needs no GPU).  Reads tests/xf_dispatch_cases.txt (key=value per line, '#' comments):
//   d_lat d_model heads enc dec ffn text_dim   the model          B Ts Tt same   the call (same=1: src and tgt are one buffer)
//   walk grid lds                              the device: layer-walking launch enabled, its workgroups, the LDS a launch may ask for
//   rows split small                           $SVG_XF_WALK_ROWS / _SPLIT / _SMALL (small=-1: unset)
//   table=1                                    with --table: also print this case's stage table
// and prints one line per case:  form Bc rows lds_bytes n_stages refusal
// --table prints, for the marked cases, the case, every stage of the first chunk's table and the workspace high-water mark.  Every field
// of a stage that is not zero is printed, a pointer as region+byte offset: a parameter by its role (enc0.in_w), the workspace as ws+offset.
// The addresses are made up, handed out in the order the forward allocates, so the offsets pin the allocation order too.
// tests/test_xf_plan_cpu.py compares both outputs with the tables recorded from the code this plan replaced.
#include "xf_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

// the model's lifecycle (latent_transformer.cpp, xf_trainer.cpp) is not linked and not called here: the plan reads the model's fields only
void XfModel::configure(const char*) {}
void XfModel::finalize(svg_ctx*, int64_t*) {}
void XfModel::weights_changed(bool) {}

// ---- made-up address space: named regions -----------------------------------------------------------------------------------------------
struct Region { std::string name; uintptr_t lo, hi; };
static std::vector<Region> g_regions;
static uintptr_t g_next = (uintptr_t)1 << 32;
// a parameter's region is named by its role: the state_dict name with its long parts abbreviated (enc0.in_w, dec1.cout_b, dec.norm.w)
static std::string role(std::string n) {
  static const char* const sub[][2] = {{"transformer.encoder.layers.", "enc"}, {"transformer.decoder.layers.", "dec"}, {"transformer.encoder.", "enc."},
      {"transformer.decoder.", "dec."}, {"self_attn.in_proj_", "in_"}, {"self_attn.out_proj.", "out_"}, {"multihead_attn.in_proj_", "cin_"},
      {"multihead_attn.out_proj.", "cout_"}, {"linear1.", "l1_"}, {"linear2.", "l2_"}, {"project_image_embedding.", "emb_"}, {"embedding.", "emb_"},
      {"weight", "w"}, {"bias", "b"}};
  for (auto& kv : sub)
    for (size_t at; (at = n.find(kv[0])) != std::string::npos;) n.replace(at, strlen(kv[0]), kv[1]);
  return n;
}
static uintptr_t region(const std::string& name, int64_t bytes) {
  const uintptr_t lo = g_next;
  g_next += (uintptr_t)((bytes + 255) / 256 * 256 + 256);
  g_regions.push_back(Region{role(name), lo, lo + (uintptr_t)bytes});
  return lo;
}
static std::string where(const void* p) {
  const uintptr_t a = (uintptr_t)p;
  for (const Region& r : g_regions)
    if (a >= r.lo && a <= r.hi) return r.name + "+" + std::to_string((unsigned long long)(a - r.lo));
  return "?";
}
// one stage: every field that is not zero / null
static void print_op(int i, const WalkOp& op) {
  printf("%d", i);
  const std::pair<const char*, int> ints[] = {{"kind", op.kind}, {"bar", op.bar}, {"M", op.M}, {"N", op.N}, {"K", op.K}, {"ld", op.ld}, {"ksplit", op.ksplit},
      {"relu", op.relu}, {"Tq", op.Tq}, {"Tk", op.Tk}, {"B", op.B}, {"heads", op.heads}, {"hd", op.hd}, {"q_ld", op.q_ld}, {"kv_ld", op.kv_ld}, {"q_span", op.q_span},
      {"kv_span", op.kv_span}, {"d_txt", op.d_txt}, {"T", op.T}, {"ldy", op.ldy}, {"ld_res", op.ld_res}, {"reuse_x", op.reuse_x}, {"perm", op.perm}};
  for (auto& kv : ints) if (kv.second) printf(" %s=%d", kv.first, kv.second);
  if (op.eps != 0.f) printf(" eps=%g", (double)op.eps);
  if (op.scale != 0.f) printf(" scale=%g", (double)op.scale);
  const std::pair<const char*, const void*> ptrs[] = {{"X", op.X}, {"W", op.W}, {"slab", op.slab}, {"bias", op.bias}, {"res", op.res}, {"Y", op.Y}, {"g1", op.g1},
      {"b1", op.b1}, {"g2", op.g2}, {"b2", op.b2}, {"Y2", op.Y2}, {"qs", op.qs}, {"ks", op.ks}, {"vs", op.vs}, {"mask", op.mask}, {"kpad", op.kpad}, {"pe", op.pe},
      {"pe_row", op.pe_row}, {"text", op.text}, {"Yln", op.Yln}};
  for (auto& kv : ptrs) if (kv.second) printf(" %s=%s", kv.first, where(kv.second).c_str());
  printf("\n");
}
// the workspace: the arena's bump allocation (256-byte alignment) over a made-up base
struct FakeArena {
  uintptr_t base; int64_t top = 0, high = 0;
  void* alloc(int64_t bytes) {
    const int64_t off = (top + 255) / 256 * 256;
    top = off + bytes;
    if (top > high) high = top;
    return (void*)(base + (uintptr_t)off);
  }
};

static std::map<std::string, long long> parse(const char* line) {
  std::map<std::string, long long> kv;
  char buf[1024];
  snprintf(buf, sizeof(buf), "%s", line);
  for (char* tok = strtok(buf, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
    if (tok[0] == '#') break;
    char* eq = strchr(tok, '=');
    if (!eq) { fprintf(stderr, "bad token '%s'\n", tok); exit(2); }
    *eq = 0;
    kv[tok] = atoll(eq + 1);
  }
  return kv;
}

int main(int argc, char** argv) {
  bool table = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) { if (!strcmp(argv[i], "--table")) table = true; else path = argv[i]; }
  FILE* f = path ? fopen(path, "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: xf_plan_dump [--table] CASES\n"); return 2; }
  char line[1024];
  while (fgets(line, sizeof(line), f)) {
    auto kv = parse(line);
    if (kv.empty()) continue;
    auto get = [&](const char* k, long long dflt) { return kv.count(k) ? kv[k] : dflt; };
    g_regions.clear();
    g_next = (uintptr_t)1 << 32;
    XfModel m;
    m.d_lat = (int)get("d_lat", 0); m.d_model = (int)get("d_model", 0); m.heads = (int)get("heads", 8); m.enc_layers = (int)get("enc", 0);
    m.dec_layers = (int)get("dec", 0); m.ffn = (int)get("ffn", 2048); m.text_dim = (int)get("text_dim", 0);
    m.each_param(m.w, [&](const std::string& name, std::initializer_list<int64_t> shape, const float*& slot) {
      int64_t n = 1;
      for (int64_t v : shape) n *= v;
      slot = (const float*)region(name, n * 4);
    });
    m.pe = (float*)region("pe", (int64_t)64 * m.d_model * 4);
    const int B = (int)get("B", 1), Ts = (int)get("Ts", 6), Tt = (int)get("Tt", 6);
    const bool same = get("same", 1) != 0;
    const XfPlan p = xf_plan(m, XfShape{B, Ts, Tt, m.text_dim > 0, same}, XfDevice{get("walk", 1) != 0, (int)get("grid", 256), get("lds", kWalkMaxLds)},
                             XfKnobs{get("rows", 96), get("split", 0), get("small", -1)});
    if (!table) { printf("%d %d %d %lld %d %d\n", p.form, p.Bc, p.rows, (long long)p.lds_bytes, p.n_stages, p.refusal); continue; }
    if (!get("table", 0) || p.form == XF_PER_GEMM) continue;
    // the first chunk, as XfModel::forward sets it up
    const int bc = std::min(B, p.Bc);
    const float* src = (const float*)region("src", (int64_t)B * Ts * m.d_lat * 4);
    const float* tgt = same ? src : (const float*)region("tgt", (int64_t)B * Tt * m.d_lat * 4);
    float* out = (float*)region("out", (int64_t)B * Tt * m.d_lat * 4);
    const float* mask = (const float*)region("mask", (int64_t)Tt * Tt * 4);
    const float* text = m.text_dim ? (const float*)region("text", (int64_t)B * m.text_dim * 4) : nullptr;
    const float* src_pad = (const float*)region("src_pad", (int64_t)B * Ts * 4);
    const float* tgt_pad = (const float*)region("tgt_pad", (int64_t)B * Tt * 4);
    const int32_t* iota = (const int32_t*)region("iota", 64 * 4);
    FakeArena arena{region("ws", (int64_t)1 << 34)};
    if (B > p.Bc) out = (float*)arena.alloc((int64_t)Tt * bc * m.d_lat * 4);
    const XfChunk c{bc, Ts, Tt, src, tgt, mask, text, src_pad, tgt_pad, iota, out};
    const XfWalkWs ws = xf_walk_workspace(m, c, p.form, [](void* u, int64_t n) { return (float*)((FakeArena*)u)->alloc(n * 4); }, &arena);
    std::vector<WalkOp> ops;
    if (p.form == XF_WALK_SMALL) xf_walk_small_table(m, c, ws, (int)get("grid", 256), ops);
    else xf_walk_table(m, c, ws, ops);
    printf("# %s", line);
    for (size_t i = 0; i < ops.size(); ++i) print_op((int)i, ops[i]);
    printf("high %lld\n", (long long)arena.high);
  }
  fclose(f);
  return 0;
}
