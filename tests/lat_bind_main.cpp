// Walks the host logic of the C ABI (sailfish_amd/csrc/slf_bind.h) for the lattices D3Q15 and D3Q27 on the CPU and prints one
// line per case:  section <tab> lattice <tab> subject <tab> code <tab> message [<tab> kernel kind]
//   config   a descriptor that is served, and one per thing the lattices do not serve: module_config()
//   resolve  every name of slf::KERNEL_TABLE asked of a served module (two-copy and in-place): resolve()
//   bind     the reference's face argument list on the box kernels: bind()
// tests/test_lat_host.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <stdio.h>

#include <functional>
#include <set>
#include <string>

#include "bind_desc.h"
#include "slf_bind.h"

namespace {

slf_module_desc base_desc(int lattice, int access) {
  slf_module_desc d = bind_base_desc(lattice);
  d.access_pattern = access;
  return d;
}

void config_line(const char* lattice, const char* subject, const slf_module_desc& d) {
  slf::ModuleConfig c;
  const char* why = "";
  const int rc = slf::module_config(&d, &c, &why);
  printf("config\t%s\t%s\t%d\t%s\tvariant=%d\n", lattice, subject, rc, rc ? why : "", rc ? -1 : c.geo.variant);
}

}  // namespace

int main() {
  const int lattices[2] = {SLF_D3Q15, SLF_D3Q27};
  const char* names[2] = {"D3Q15", "D3Q27"};
  for (int l = 0; l < 2; l++) {
    const int lat = lattices[l];
    const char* ln = names[l];
    struct Case { const char* subject; std::function<void(slf_module_desc&)> change; };
    const Case cases[] = {
        {"served", [](slf_module_desc&) {}},
        {"served-aa-f64-force-edm-incompressible", [](slf_module_desc& d) {
           d.access_pattern = SLF_AA; d.precision = 8; d.has_force = 1; d.accel[0] = 1e-5; d.force_implementation = SLF_FORCE_EDM;
           d.incompressible = SLF_DENSITY_INCOMPRESSIBLE; }},
        {"mrt", [](slf_module_desc& d) { d.model = SLF_MRT; }},
        {"elbm", [](slf_module_desc& d) { d.model = SLF_ELBM; }},
        {"regularized", [](slf_module_desc& d) { d.regularized = 1; }},
        {"subgrid", [](slf_module_desc& d) { d.subgrid = SLF_SUBGRID_LES_SMAGORINSKY; d.smagorinsky_const = 0.1; }},
        {"minimize_roundoff", [](slf_module_desc& d) { d.incompressible = SLF_DENSITY_ROUNDOFF; }},
        {"indirect", [](slf_module_desc& d) { d.node_addressing = SLF_ADDR_INDIRECT; d.dist_stride = 100; }},
        {"shan-chen-binary", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_BINARY; }},
        {"shan-chen-single", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_SINGLE; }},
        {"free-energy", [](slf_module_desc& d) { d.simtype = SLF_SIM_FREE_ENERGY; }},
        {"ternary", [](slf_module_desc& d) { d.simtype = SLF_SIM_SHAN_CHEN_TERNARY; }},
    };
    for (const Case& c : cases) {
      slf_module_desc d = base_desc(lat, SLF_AB);
      c.change(d);
      config_line(ln, c.subject, d);
    }
    for (int kind = SLF_NK_REGULARIZED_VELOCITY; kind <= SLF_NK_WALL_TMS; kind++) {
      slf_module_desc d = base_desc(lat, SLF_AB);
      d.type_kind[5] = kind;
      config_line(ln, ("node-kind-" + std::to_string(kind)).c_str(), d);
    }
    for (int access : {SLF_AB, SLF_AA}) {
      const slf_module_desc d = base_desc(lat, access);
      slf::ModuleConfig c;
      const char* why = "";
      if (slf::module_config(&d, &c, &why)) return 2;
      std::set<std::string> seen;
      for (const slf::KernelRow& r : slf::KERNEL_TABLE) {
        if (!seen.insert(r.name).second) continue;
        const slf::KernelRow* row = nullptr;
        std::string err;
        const int rc = slf::resolve(c, r.name, &row, &err);
        printf("resolve\t%s\t%s-%s\t%d\t%s\t%d\n", ln, r.name, access == SLF_AB ? "ab" : "aa", rc, rc ? err.c_str() : "",
               rc ? -1 : (int)row->kind);
      }
      // the reference's own face argument list on a box kernel
      const slf::KernelRow* row = nullptr;
      std::string err;
      if (slf::resolve(c, "CollectContinuousData", &row, &err)) return 3;
      unsigned long long p0 = 4096, p1 = 8192;
      int32_t i[5] = {2, 0, 1, 6, 10};
      const void* argv[7] = {&p0, &i[0], &i[1], &i[2], &i[3], &i[4], &p1};
      slf::BoundArgs b;
      const int rc = slf::bind(c, *row, "PiiiiiP", argv, 7, &b, &err);
      printf("bind\t%s\tCollectContinuousData-reference-form-%s\t%d\t%s\n", ln, access == SLF_AB ? "ab" : "aa", rc, rc ? err.c_str() : "");
    }
  }
  // any other id stays unknown (D3Q13 would be 4 if it existed)
  for (int lat : {4, 7}) {
    const slf_module_desc d = base_desc(lat, SLF_AB);
    config_line(std::to_string(lat).c_str(), "unknown", d);
  }
  return 0;
}
