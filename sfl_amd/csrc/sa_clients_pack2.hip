// sa_clients_pack2.hip — the packed (kPacked, two 32-bit values per ring
// word) float32 instantiations of the masking kernel: one party with its wire
// image (sa_mask_pack2: 0..16 streams) and 2..8 co-located parties, with
// digests / wire images or sum-only (sa_fused_clients_pack2).  Not
// instantiated: continue mode, weight vectors, fused DP, the cross-GPU
// shapes, the bipartite schedule.  A translation unit of its own: its 31
// heavy kernels compile beside sa_clients_f32.hip's instead of after them,
// and it alone is built with packed-fp32 arithmetic switched off (Makefile,
// PACK2_FLAGS; what that does and does not change: DESIGN.md §21).
#include "sa_clients_impl.h"
#include "sa_registry.h"

namespace sa {

#define P2(L, X, K) SA_ENTRY_K(float, float, SA_F32, SA_F32, L, X, (K) | kPacked)
#define P1(X) P2(1, X, kLean1)
LaunchFn find_pack2_kernel(int L, int X, int K) {
  static const KernelEntry kEntries[] = {
    P1(0), P1(1), P1(2),  P1(3),  P1(4),  P1(5),  P1(6),  P1(7),  P1(8),
    P1(9), P1(10), P1(11), P1(12), P1(13), P1(14), P1(15), P1(16),
    P2(2, 0, 0), P2(3, 0, 0), P2(4, 0, 0), P2(5, 0, 0), P2(6, 0, 0), P2(7, 0, 0), P2(8, 0, 0),
    P2(2, 0, kSumOnly), P2(3, 0, kSumOnly), P2(4, 0, kSumOnly), P2(5, 0, kSumOnly), P2(6, 0, kSumOnly),
    P2(7, 0, kSumOnly), P2(8, 0, kSumOnly),
  };
  for (const KernelEntry& e : kEntries)
    if (e.L == L && e.X == X && e.K == (K | kPacked)) return e.fn;
  return nullptr;
}
#undef P1
#undef P2

}  // namespace sa
