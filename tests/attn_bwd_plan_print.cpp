// Prints tim_amd/csrc/attn_bwd_plan.h's answer - the LDS plan of the co-resident fused attention backward, the helper its
// launcher uses - for the shapes it reads from stdin, one `<S> <F> <Dh>` per line (tests/test_attn_bwd_plan.py).
#include <cstdio>

#include "attn_bwd_plan.h"

int main() {
  int S, F, Dh;
  while (scanf("%d %d %d", &S, &F, &Dh) == 3) {
    const AttnBwdCoPlan p = attn_bwd_co_plan(S, F, Dh);
    printf("fits=%d kv_rows=%d sweeps=%d k_off=%zu v_off=%zu ds_off=%zu pt_off=%zu lds=%zu\n", (int)p.fits, p.kv_rows, p.sweeps, p.k_off,
           p.v_off, p.ds_off, p.pt_off, p.lds_bytes);
  }
  return 0;
}
