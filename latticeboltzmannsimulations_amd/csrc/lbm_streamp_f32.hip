// lbm_streamp_f32.hip -- explicit instantiations of the streaming kernel with two rows per wave (k_stream_pairs), float (lbm_inst.hpp)
#define LBM_INST LBM_INST_STREAMP(float)
#include "lbm_inst.hpp"
