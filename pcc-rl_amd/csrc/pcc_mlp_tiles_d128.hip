// pcc_mlp_tiles_d128.hip -- the tiled gradient and forward kernels of pcc_mlp_tiles.h for observation lengths padded to 128, their
// three hidden classes: a translation unit per length class, so that the classes compile side by side.
#include "pcc_mlp_tiles.h"

namespace pcc_tiles {
int launch_grad_d128(const GradArgs &a, hipStream_t st, int *blocks_out) { return launch_d<128>(a, st, blocks_out); }
int launch_act_d128(const ActArgs &a, hipStream_t st) { return launch_d<128>(a, st); }
}  // namespace pcc_tiles
