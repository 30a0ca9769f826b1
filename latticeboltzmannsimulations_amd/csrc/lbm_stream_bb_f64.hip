// lbm_stream_bb_f64.hip -- explicit instantiations of the strip-streaming multi-step kernel (k_stream) with bounce-back walls, double (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAM_BB(double)
#include "lbm_inst.hpp"
