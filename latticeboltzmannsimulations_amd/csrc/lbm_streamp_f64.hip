// lbm_streamp_f64.hip -- explicit instantiations of the streaming kernel with two rows per wave (k_stream_pairs), double (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMP(double)
#include "lbm_inst.hpp"
