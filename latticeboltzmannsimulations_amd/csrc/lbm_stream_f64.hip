// lbm_stream_f64.hip -- explicit instantiations of the strip-streaming multi-step kernel (k_stream), double (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAM(double)
#include "lbm_inst.hpp"
