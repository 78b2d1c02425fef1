// agg_plain_bernoulli.hip — instantiations of agg_plain_kernel for noise kind "bernoulli" (see agg_plain.hpp).
#include "agg_plain.hpp"

namespace stag {
template <>
void agg_launch_plain<kBernoulli>(const AggArgs& a, int lpe, bool walk, dim3 grid, hipStream_t stream) {
  agg_launch_plain_impl<kBernoulli>(a, lpe, walk, grid, stream);
}
}  // namespace stag
