// Walks the host logic of the C ABI (sailfish_amd/csrc/slf_bind.h) for shallow-water modules (slf_module_desc::equilibrium =
// SLF_EQ_SHALLOW_WATER) on the CPU and prints one line per case:
//   section <tab> subject <tab> code <tab> message <tab> details
//   config   the descriptors that are served and one per thing the model is refused with: module_config()
//   resolve  every name of slf::KERNEL_TABLE asked of a served module and of the same module with the polynomial: resolve()
// tests/test_sw_bind.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <stdio.h>

#include <functional>
#include <set>
#include <string>

#include "bind_desc.h"
#include "slf_bind.h"

namespace {

slf_module_desc base_desc() {
  slf_module_desc d = bind_base_desc(SLF_D2Q9);
  d.type_kind[d.n_types++] = SLF_NK_SLIP;
  d.equilibrium = SLF_EQ_SHALLOW_WATER;
  d.gravity = 0.05;
  return d;
}

void config_line(const char* subject, const slf_module_desc& d) {
  slf::ModuleConfig c;
  const char* why = "";
  const int rc = slf::module_config(&d, &c, &why);
  printf("config\t%s\t%d\t%s\tvariant=%d equilibrium=%d gravity=%g has_force=%d accel_field=%d block_x=%d\n", subject, rc, rc ? why : "",
         rc ? -1 : c.geo.variant, rc ? -1 : c.phys.equilibrium, rc ? -1.0 : c.phys.gravity, rc ? -1 : c.phys.has_force,
         rc ? -1 : c.phys.accel_field, rc ? -1 : c.block_x);
}

}  // namespace

int main() {
  struct Case { const char* subject; std::function<void(slf_module_desc&)> change; };
  const Case cases[] = {
      {"served", [](slf_module_desc&) {}},
      {"served-aa-f64", [](slf_module_desc& d) { d.access_pattern = SLF_AA; d.precision = 8; }},
      {"served-fluid-only", [](slf_module_desc& d) { d.fluid_only = 1; d.n_types = 0; }},
      {"served-wide", [](slf_module_desc& d) { d.lat_nx = 1002; d.arr_nx = 1024; }},
      {"served-wide-field", [](slf_module_desc& d) { d.lat_nx = 1002; d.arr_nx = 1024; d.accel_field = 1; }},
      {"served-force-edm", [](slf_module_desc& d) { d.has_force = 1; d.accel[0] = 1e-5; d.force_implementation = SLF_FORCE_EDM; }},
      {"served-field", [](slf_module_desc& d) { d.accel_field = 1; }},
      {"polynomial", [](slf_module_desc& d) { d.equilibrium = SLF_EQ_BGK; d.gravity = 0.0; }},
      {"polynomial-ignores-gravity", [](slf_module_desc& d) { d.equilibrium = SLF_EQ_BGK; }},
      {"polynomial-wide", [](slf_module_desc& d) { d.equilibrium = SLF_EQ_BGK; d.gravity = 0.0; d.lat_nx = 1002; d.arr_nx = 1024; }},
      {"bad-equilibrium", [](slf_module_desc& d) { d.equilibrium = 2; }},
      {"negative-equilibrium", [](slf_module_desc& d) { d.equilibrium = -1; }},
      {"zero-gravity", [](slf_module_desc& d) { d.gravity = 0.0; }},
      {"negative-gravity", [](slf_module_desc& d) { d.gravity = -0.05; }},
      {"d3q19", [](slf_module_desc& d) { d.lattice = SLF_D3Q19; d.lat_nz = 4; d.arr_nz = 4; }},
      {"d3q15", [](slf_module_desc& d) { d.lattice = SLF_D3Q15; d.lat_nz = 4; d.arr_nz = 4; }},
      {"mrt", [](slf_module_desc& d) { d.model = SLF_MRT; }},
      {"elbm", [](slf_module_desc& d) { d.model = SLF_ELBM; }},
      {"entropic_equilibrium", [](slf_module_desc& d) { d.entropic_equilibrium = 1; }},
      {"regularized", [](slf_module_desc& d) { d.regularized = 1; }},
      {"subgrid", [](slf_module_desc& d) { d.subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d.smagorinsky_const = 0.1; }},
      {"minimize_roundoff", [](slf_module_desc& d) { d.incompressible = SLF_DENSITY_ROUNDOFF; }},
      {"incompressible", [](slf_module_desc& d) { d.incompressible = SLF_DENSITY_INCOMPRESSIBLE; }},
      {"indirect", [](slf_module_desc& d) { d.node_addressing = SLF_ADDR_INDIRECT; d.dist_stride = 100; }},
      {"tms", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_WALL_TMS; }},
      {"equilibrium-density-node", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_EQUILIBRIUM_DENSITY; }},
      {"zouhe-velocity-node", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_ZOUHE_VELOCITY; }},
      {"regularized-velocity-node", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_REGULARIZED_VELOCITY; }},
      {"copy-node", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_COPY; }},
      {"do-nothing-node", [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_DO_NOTHING; d.access_pattern = SLF_AA; }},
      {"shan-chen-binary", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_BINARY; }},
      {"shan-chen-single", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_SINGLE; }},
      {"free-energy", [](slf_module_desc& d) { d.simtype = SLF_SIM_FREE_ENERGY; }},
      {"ternary", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_TERNARY; }},
  };
  for (const Case& c : cases) {
    slf_module_desc d = base_desc();
    c.change(d);
    config_line(c.subject, d);
  }
  // the kernel names of a served module: the resident kernel is refused by name, the rest resolves as with the polynomial
  for (int sw : {1, 0}) {
    slf_module_desc d = base_desc();
    if (!sw) { d.equilibrium = SLF_EQ_BGK; d.gravity = 0.0; }
    d.fluid_only = 1; d.n_types = 0;
    d.periodic_fused[0] = d.periodic_fused[1] = 1;
    slf::ModuleConfig c;
    const char* why = "";
    if (slf::module_config(&d, &c, &why)) return 2;
    std::set<std::string> seen;
    for (const slf::KernelRow& r : slf::KERNEL_TABLE) {
      if (!seen.insert(r.name).second) continue;
      const slf::KernelRow* row = nullptr;
      std::string err;
      const int rc = slf::resolve(c, r.name, &row, &err);
      printf("resolve\t%s-%s\t%d\t%s\t%d\n", r.name, sw ? "sw" : "plain", rc, rc ? err.c_str() : "", rc ? -1 : (int)row->kind);
    }
  }
  return 0;
}
