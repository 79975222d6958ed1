// Host-only probe of csrc/gemm_select.h for tests/test_gemm_select_cpu.py: reads shape lines from stdin (formats in
// tests/golden/make_golden_gemm_select.py) and prints `input | choice per precision` (columns in the header of
// tests/golden/gemm_select_table.txt).  The launch parameters are filled as the entry points of gemm.hip fill them.
#include "dm4d.h"
#include "gemm_select.h"

#include <stdio.h>
#include <string.h>

namespace {

u16 g_mem[8];     // stands for every device pointer: nothing is dereferenced
float g_ws[1];

void print_choice(const GemmChoice& c) {
  if (c.id) printf(" %d/%d", c.id, c.splits);
  else printf(" unsupported");
}

template <bool CONV>
GemmChoice pick(GemmParams p, int prec, bool with_ws, int B, bool* bad) {
  if (prec == PREC_PAR) p.flags |= DM4D_EPI_F32SIDE;
  if (prec == PREC_H16) p.flags |= DM4D_EPI_H16;
  p.ws = with_ws && strip_ws_bytes(p, B) ? g_ws : nullptr;
  const GemmChoice c = select_cfg<CONV>(p, prec);
  if (prec == PREC_PAR && c.id && !par_has_id(CONV, c.id)) *bad = true;  // an id PAR = 1 is not instantiated for
  return c;
}

}  // namespace

int main() {
  char line[256];
  bool bad = false;
  while (fgets(line, sizeof line, stdin)) {
    line[strcspn(line, "\n")] = 0;
    if (!line[0] || line[0] == '#') continue;
    GemmParams p{};
    p.A = g_mem; p.Wt = g_mem; p.C = g_mem; p.out_scale = 1.0f;
    int B, H, W, Cin, Cout, stride, up, M, N, K, K1, geglu;
    if (sscanf(line, "g %d %d %d %d %d", &M, &N, &K, &K1, &geglu) == 5) {
      p.lda = K1 ? K1 : K; p.A2 = K1 ? g_mem : nullptr; p.lda2 = K1 ? K - K1 : 0; p.K1 = K1;
      p.ldw = K; p.ldc = N; p.M = M; p.N = N; p.K = K; p.rows_per_rb = 1; p.flags = geglu ? DM4D_EPI_GEGLU : 0;
      printf("%s |", line);
      for (int prec = PREC_FAST; prec <= PREC_H16; ++prec) print_choice(pick<false>(p, prec, false, 0, &bad));
    } else if (sscanf(line, "c %d %d %d %d %d %d %d", &B, &H, &W, &Cin, &Cout, &stride, &up) == 7) {
      const int pad = 1, Ho = ((up ? 2 * H : H) + 2 * pad - 3) / stride + 1, Wo = ((up ? 2 * W : W) + 2 * pad - 3) / stride + 1;
      p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.stride = stride; p.pad = pad; p.upsample = up;
      p.ldw = (int64_t)9 * Cin; p.ldc = Cout; p.M = B * Ho * Wo; p.N = Cout; p.K = 9 * Cin; p.rows_per_rb = Ho * Wo;
      GemmParams h = p;
      h.flags |= DM4D_EPI_H16;
      if (strip_ws_bytes(p, B) != strip_ws_bytes(h, B)) bad = true;  // one workspace serves both precisions (host/ops.py sizes it once)
      printf("%s |", line);
      print_choice(pick<true>(p, PREC_FAST, false, B, &bad));
      print_choice(pick<true>(p, PREC_FAST, true, B, &bad));
      printf(" %zu", strip_ws_bytes(p, B));
      GemmParams q = p;  // the parity precision is offered the fast precision's workspace and must not take it
      q.ws = strip_ws_bytes(p, B) ? g_ws : nullptr;
      q.flags |= DM4D_EPI_F32SIDE;
      const GemmChoice par = select_cfg<true>(q, PREC_PAR);
      print_choice(par);
      if (par.id && !par_has_id(true, par.id)) bad = true;
      print_choice(pick<true>(p, PREC_H16, false, B, &bad));
      print_choice(pick<true>(p, PREC_H16, true, B, &bad));
    } else if (sscanf(line, "u %d %d %d %d %d", &B, &H, &W, &Cin, &Cout) == 5) {
      p.H = H; p.W = W; p.Cin = Cin; p.Ho = H; p.Wo = W; p.stride = 1; p.pad = 1;
      p.ldw = (int64_t)4 * Cin; p.ldc = Cout; p.M = B * H * W; p.N = Cout; p.K = 4 * Cin; p.rows_per_rb = H * W; p.up_w = W;
      const int id = choose_up2x(p);
      printf("%s | %s", line, id == 32 ? "256x128" : id == 31 ? "128x128" : id == 33 ? "128x64" : "?");
    } else {
      fprintf(stderr, "gemm_select_probe: bad line: %s\n", line);
      return 2;
    }
    printf("\n");
  }
  if (bad) fprintf(stderr, "gemm_select_probe: inconsistent selection (parity id without a kernel, or workspace rules that differ)\n");
  return bad ? 3 : 0;
}
