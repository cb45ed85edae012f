// Host-only dump of the sampling loop's schedule plan (csrc/sampler_plan.cpp, which holds no kernel and makes no HIP call: this builds in
// seconds and needs no GPU).  Reads tests/sampler_plan_cases.txt (key=value per line, '#' comments):
//   sampler steps start      the arguments of sampler_plan()
// and prints per case one line with the plan's scalars, floats as their bit patterns,
//   plan sampler= steps= start= add_noise= noise_sa= noise_s1a= z_scale= scaled_input= state=
// followed by one line per row, `i` and its eight floats as hexadecimal bit patterns; a refused case prints `refused: <message>` alone.
// tests/test_sampler_plan_cpu.py compares the output with the rows recorded from the code this plan replaced.
#include "sampler_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <string>

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: sampler_plan_dump CASES\n"); return 2; }
  char line[256];
  while (fgets(line, sizeof(line), f)) {
    std::map<std::string, int> kv;
    for (char* tok = strtok(line, " \t\r\n"); tok && tok[0] != '#'; tok = strtok(nullptr, " \t\r\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) { fprintf(stderr, "bad token '%s'\n", tok); return 2; }
      *eq = 0;
      kv[tok] = atoi(eq + 1);
    }
    if (kv.empty()) continue;
    try {
      const SamplerPlan p = sampler_plan(kv["sampler"], kv["steps"], kv["start"]);
      printf("plan sampler=%d steps=%d start=%d add_noise=%d noise_sa=%08x noise_s1a=%08x z_scale=%08x scaled_input=%d state=%d\n", p.sampler,
             p.num_steps, p.start_step, (int)p.add_noise, bits(p.noise_sa), bits(p.noise_s1a), bits(p.z_scale), (int)p.scaled_input,
             p.state_buffers);
      for (int i = 0; i < p.num_steps; ++i) {
        printf("%d", i);
        for (int j = 0; j < kSamplerRow; ++j) printf(" %08x", bits(p.row(i)[j]));
        printf("\n");
      }
    } catch (const std::exception& e) {
      printf("refused: %s\n", e.what());
    }
  }
  fclose(f);
  return 0;
}
