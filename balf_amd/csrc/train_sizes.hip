// balf_train_unit_sizes (include/balf_hip.h): the workspace and saved bytes of a training unit at a channel width, ONE query for
// the units that take their width as an argument.  Each unit states its layout once, in its own file, and hands its sizes out
// through <unit>_train_sizes; this file only picks the unit.
#include "common.h"

namespace balf {
int rcab_train_sizes(int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes);   // rcab_train.hip
int gmlp_train_sizes(int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes);   // gmlp_train.hip
int pool_train_sizes(int C, int B, int H, int W, size_t *workspace_bytes, size_t *saved_bytes);     // pool_train.hip
}  // namespace balf

extern "C" int balf_train_unit_sizes(int unit, int C, int B, int Hc, int Wc, size_t *workspace_bytes, size_t *saved_bytes) {
    if (!workspace_bytes || !saved_bytes) return BALF_ERR_ARG;
    switch (unit) {
        case BALF_UNIT_RCAB: return balf::rcab_train_sizes(C, B, Hc, Wc, workspace_bytes, saved_bytes);
        case BALF_UNIT_GMLP: return balf::gmlp_train_sizes(C, B, Hc, Wc, workspace_bytes, saved_bytes);
        case BALF_UNIT_POOL: return balf::pool_train_sizes(C, B, Hc, Wc, workspace_bytes, saved_bytes);
        default: return BALF_ERR_ARG;
    }
}
