// Walks the rule of the per-node sweep's variants (sailfish_amd/csrc/slf_variant.h) on the CPU, through module_config()
// (slf_bind.h), over the cross product of the descriptor members that select a variant, and prints
//   checked <tab> descriptors <tab> accepted
//   fail <tab> what <tab> descriptor                        one per broken property, none when all is well
//   variants <tab> lattice <tab> precision <tab> count      the distinct per-node variants the accepted descriptors reach
//   total <tab> count
// (a) every variant an accepted descriptor can launch exists, and its block_x is within that variant's launch bound;
// (b) the variants reached are exactly the ones that exist, i.e. the ones launch_sweep2 (slf_kernels.hip) instantiates.
// tests/test_variant_rule.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <stdio.h>

#include <set>
#include <string>
#include <tuple>

#include "slf_bind.h"

namespace {

using Key = std::tuple<int, int, int, int, bool, bool, bool, bool, bool, bool, bool>;
Key key_of(int lattice, int precision, const slf::SweepVariant& v) {
  return Key(lattice, precision, v.model, v.prop, v.general, v.indirect, v.roundoff, v.turb, v.tms, v.accf, v.sw);
}

// the smallest box the header accepts (nx = 6), or a row wider than any launch bound (nx = 1002)
slf_module_desc base_desc(int lattice, int nx) {
  slf_module_desc d = {};
  d.struct_size = sizeof(slf_module_desc);
  d.lattice = lattice;
  d.lat_nx = nx; d.lat_ny = 6; d.lat_nz = lattice == SLF_D2Q9 ? 1 : 6;
  d.arr_nx = nx + 2; d.arr_ny = 6; d.arr_nz = d.lat_nz;
  d.envelope = 1;
  d.relaxation_enabled = 1;
  d.tau = 0.8; d.visc = 0.1;
  d.nt_type_mask = 7; d.nt_misc_shift = 3;
  d.n_types = 6;
  for (int i = 0; i < 6; i++) d.type_kind[i] = i;      // fluid, ghost, unused, propagation-only, full-way, half-way
  d.smagorinsky_const = 0.1;
  d.entropy_tolerance = 1e-6; d.alpha_tolerance = 1e-10;
  d.gravity = 0.05;
  return d;
}

}  // namespace

int main() {
  std::set<Key> reached, existing;
  long checked = 0, accepted = 0, failures = 0;
  for (int lattice : {SLF_D2Q9, SLF_D3Q19}) for (int precision : {4, 8}) for (int model : {SLF_BGK, SLF_MRT, SLF_ELBM})
  for (int access : {SLF_AB, SLF_AA}) for (int fluid_only : {0, 1}) for (int addressing : {SLF_ADDR_DIRECT, SLF_ADDR_INDIRECT})
  for (int density : {SLF_DENSITY_COMPRESSIBLE, SLF_DENSITY_INCOMPRESSIBLE, SLF_DENSITY_ROUNDOFF})
  for (int regularized : {0, 1}) for (int subgrid : {SLF_SUBGRID_NONE, SLF_SUBGRID_LES_SMAGORINSKY}) for (int tms : {0, 1})
  for (int accel_field : {0, 1}) for (int equilibrium : {SLF_EQ_BGK, SLF_EQ_SHALLOW_WATER}) for (int nx : {6, 1002}) {
    slf_module_desc d = base_desc(lattice, nx);
    d.precision = precision; d.model = model; d.access_pattern = access; d.fluid_only = fluid_only;
    d.node_addressing = addressing;
    if (addressing == SLF_ADDR_INDIRECT) d.dist_stride = 100;
    d.incompressible = density; d.regularized = regularized; d.subgrid = subgrid;
    if (tms) d.type_kind[5] = SLF_NK_WALL_TMS;
    d.accel_field = accel_field; d.equilibrium = equilibrium;
    char name[200];
    snprintf(name, sizeof name, "lattice=%d precision=%d model=%d access=%d fluid_only=%d addressing=%d incompressible=%d "
             "regularized=%d subgrid=%d tms=%d accel_field=%d equilibrium=%d nx=%d", lattice, precision, model, access, fluid_only,
             addressing, density, regularized, subgrid, tms, accel_field, equilibrium, nx);
    slf::ModuleConfig c;
    const char* why = "";
    checked++;
    if (slf::module_config(&d, &c, &why) != SLF_OK) continue;
    accepted++;
    for (slf::Prop prop : {slf::PROP_AB, slf::PROP_AA_EVEN, slf::PROP_AA_ODD}) {
      if ((prop == slf::PROP_AB) != (access == SLF_AB)) continue;
      const slf::SweepVariant v = slf::per_node_variant_of(c.sel, c.geo, c.phys, prop);
      if (const char* rule = slf::per_node_variant_conflict(lattice, v)) {
        printf("fail\taccepted, but %s\t%s prop=%d\n", rule, name, (int)prop);
        failures++;
        continue;
      }
      if (c.block_x > slf::sweep_max_threads(v)) {
        printf("fail\tblock_x %d above the launch bound %d\t%s prop=%d\n", c.block_x, slf::sweep_max_threads(v), name, (int)prop);
        failures++;
      }
      reached.insert(key_of(lattice, precision, v));
    }
  }
  printf("checked\t%ld\t%ld\n", checked, accepted);
  // what launch_sweep2 instantiates: every value of the fields its picks range over, where the rule says "exists"
  for (int lattice : {SLF_D2Q9, SLF_D3Q19}) for (int precision : {4, 8}) {
    for (int bits = 0; bits < 9 * 128; bits++) {
      slf::SweepVariant v;
      v.model = (bits >> 7) % 3; v.prop = (bits >> 7) / 3;
      v.general = bits & 1; v.indirect = bits & 2; v.roundoff = bits & 4; v.turb = bits & 8; v.tms = bits & 16; v.accf = bits & 32;
      v.sw = bits & 64;
      if (slf::per_node_variant_exists(lattice, v)) existing.insert(key_of(lattice, precision, v));
    }
    long n = 0;
    for (const Key& k : reached) n += std::get<0>(k) == lattice && std::get<1>(k) == precision;
    printf("variants\t%d\t%d\t%ld\n", lattice, precision, n);
  }
  for (const Key& k : existing) {
    if (!reached.count(k)) {
      printf("fail\tinstantiated, but no accepted descriptor reaches it\tlattice=%d precision=%d model=%d prop=%d general=%d indirect=%d "
             "roundoff=%d turb=%d tms=%d accf=%d sw=%d\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k),
             (int)std::get<4>(k), (int)std::get<5>(k), (int)std::get<6>(k), (int)std::get<7>(k), (int)std::get<8>(k),
             (int)std::get<9>(k), (int)std::get<10>(k));
      failures++;
    }
  }
  for (const Key& k : reached) failures += existing.count(k) ? 0 : 1;      // (reported above: "accepted, but ...")
  printf("total\t%zu\n", reached.size());
  return failures ? 1 : 0;
}
