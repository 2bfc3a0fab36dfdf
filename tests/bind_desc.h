// The descriptors the stand-alone bind programs (tests/*_bind_main.cpp) start from.  Each program sets the fields in which
// its cases differ.
#pragma once
#include "slf_bind.h"

// A valid single-fluid BGK module that reads no node map: 6 x 5 (x 4 unless D2Q9) nodes in single precision, two-copy access
// pattern, rows padded to 8.
inline slf_module_desc bind_fluid_only_desc(int lattice) {
  slf_module_desc d = {};
  d.struct_size = sizeof(slf_module_desc);
  d.lattice = lattice; d.model = SLF_BGK; d.precision = 4; d.access_pattern = SLF_AB;
  d.lat_nx = 6; d.lat_ny = 5; d.lat_nz = lattice == SLF_D2Q9 ? 1 : 4;
  d.arr_nx = 8; d.arr_ny = 5; d.arr_nz = d.lat_nz;
  d.envelope = 1;
  d.relaxation_enabled = 1;
  d.tau = 0.8; d.visc = 0.1;
  d.fluid_only = 1;
  return d;
}

// ... with a node map of fluid, ghost, unused, propagation-only, full-way and half-way bounce-back nodes, and valid parameters
// of every model, so that a case can switch to one by its simtype alone
inline slf_module_desc bind_base_desc(int lattice) {
  slf_module_desc d = bind_fluid_only_desc(lattice);
  d.fluid_only = 0;
  d.nt_type_mask = 7; d.nt_misc_shift = 3;
  d.n_types = 6;
  for (int i = 0; i < 6; i++) d.type_kind[i] = i;
  d.tau_phi = 0.9; d.tau_theta = 1.1;
  d.fe_Gamma = 0.5; d.fe_kappa = 0.04; d.fe_A = 0.03; d.fe_tau_a = 0.9; d.fe_tau_b = 0.7; d.bc_wall_grad_order = 1;
  d.entropy_tolerance = 1e-6; d.alpha_tolerance = 1e-10;
  return d;
}
