// Walks the host logic of the C ABI (sailfish_amd/csrc/slf_bind.h) for modules with an acceleration field
// (slf_module_desc::accel_field) on the CPU and prints one line per case:
//   section <tab> subject <tab> code <tab> message <tab> details
//   config   the descriptors that are served and one per thing the field is refused with: module_config()
//   resolve  every name of slf::KERNEL_TABLE asked of a served module: resolve()
// tests/test_accf_bind.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <stdio.h>

#include <functional>
#include <set>
#include <string>

#include "bind_desc.h"
#include "slf_bind.h"

namespace {

slf_module_desc base_desc(int lattice) {
  slf_module_desc d = bind_base_desc(lattice);
  d.accel_field = 1;
  return d;
}

void config_line(const char* subject, const slf_module_desc& d) {
  slf::ModuleConfig c;
  const char* why = "";
  const int rc = slf::module_config(&d, &c, &why);
  printf("config\t%s\t%d\t%s\tvariant=%d has_force=%d accel_field=%d\n", subject, rc, rc ? why : "", rc ? -1 : c.geo.variant,
         rc ? -1 : c.phys.has_force, rc ? -1 : c.phys.accel_field);
}

}  // namespace

int main() {
  struct Case { const char* subject; int lattice; std::function<void(slf_module_desc&)> change; };
  const Case cases[] = {
      {"served-d2q9", SLF_D2Q9, [](slf_module_desc&) {}},
      {"served-d3q19", SLF_D3Q19, [](slf_module_desc&) {}},
      {"served-d3q19-mrt-aa-f64", SLF_D3Q19, [](slf_module_desc& d) { d.model = SLF_MRT; d.access_pattern = SLF_AA; d.precision = 8; }},
      {"served-d2q9-edm-incompressible-uniform-part", SLF_D2Q9, [](slf_module_desc& d) {
         d.force_implementation = SLF_FORCE_EDM; d.incompressible = SLF_DENSITY_INCOMPRESSIBLE; d.has_force = 1; d.accel[1] = 1e-5; }},
      {"served-d3q19-fluid-only", SLF_D3Q19, [](slf_module_desc& d) { d.fluid_only = 1; d.n_types = 0; }},
      {"served-d3q19-boundary-conditions", SLF_D3Q19, [](slf_module_desc& d) {
         d.nt_type_mask = 15; d.nt_misc_shift = 4; d.n_types = 16;
         for (int i = 0; i < 16; i++) d.type_kind[i] = i; }},      // everything up to SLF_NK_SLIP
      {"no-field-d3q19", SLF_D3Q19, [](slf_module_desc& d) { d.accel_field = 0; }},
      {"bad-flag", SLF_D3Q19, [](slf_module_desc& d) { d.accel_field = 2; }},
      {"d3q15", SLF_D3Q15, [](slf_module_desc&) {}},
      {"d3q27", SLF_D3Q27, [](slf_module_desc&) {}},
      {"elbm", SLF_D3Q19, [](slf_module_desc& d) { d.model = SLF_ELBM; }},
      {"regularized", SLF_D3Q19, [](slf_module_desc& d) { d.regularized = 1; }},
      {"subgrid", SLF_D3Q19, [](slf_module_desc& d) { d.subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d.smagorinsky_const = 0.1; }},
      {"minimize_roundoff", SLF_D3Q19, [](slf_module_desc& d) { d.incompressible = SLF_DENSITY_ROUNDOFF; }},
      {"tms", SLF_D3Q19, [](slf_module_desc& d) { d.type_kind[5] = SLF_NK_WALL_TMS; }},
      {"indirect", SLF_D3Q19, [](slf_module_desc& d) { d.node_addressing = SLF_ADDR_INDIRECT; d.dist_stride = 100; }},
      {"shan-chen-binary", SLF_D3Q19, [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_BINARY; }},
      {"shan-chen-single", SLF_D3Q19, [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_SINGLE; }},
      {"free-energy", SLF_D3Q19, [](slf_module_desc& d) { d.simtype = SLF_SIM_FREE_ENERGY; }},
      {"ternary", SLF_D3Q19, [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_TERNARY; }},
      {"mrt-edm", SLF_D3Q19, [](slf_module_desc& d) { d.model = SLF_MRT; d.force_implementation = SLF_FORCE_EDM; }},
  };
  for (const Case& c : cases) {
    slf_module_desc d = base_desc(c.lattice);
    c.change(d);
    config_line(c.subject, d);
  }
  // the kernel names of a served 2-D module: the resident kernel is refused by name, the rest resolves as without a field
  for (int field : {1, 0}) {
    slf_module_desc d = base_desc(SLF_D2Q9);
    d.accel_field = field;
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
      printf("resolve\t%s-%s\t%d\t%s\t%d\n", r.name, field ? "field" : "plain", rc, rc ? err.c_str() : "", rc ? -1 : (int)row->kind);
    }
  }
  return 0;
}
