// Single translation unit of libvbmc_hip.so: the kernels live in headers shared by the ABI files.
#include "abi_elbo.hip"
#include "abi_gp.hip"
#include "abi_gp_train.hip"
#include "abi_acq_search.hip"
#include "abi_is_sample.hip"
#include "abi_is_setup.hip"
#include "abi_vp_tools.hip"
#include "abi_comm.hip"
