// Walks the argument checks of the immersed boundary entry points (slf_ibm_*; sailfish_amd/csrc/slf_bind.h ibm_check) on the
// CPU and prints one line per case:  subject <tab> code <tab> message.
// tests/test_ibm_host.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <stdio.h>

#include <string>

#include "bind_desc.h"
#include "slf_bind.h"

namespace {

slf_module_desc base_desc(int lattice) {
  slf_module_desc d = bind_fluid_only_desc(lattice);
  d.accel_field = (lattice == SLF_D2Q9 || lattice == SLF_D3Q19) ? 1 : 0;
  return d;
}

struct Call {
  bool has_field = true;
  int n = 130;
  int32_t origin[3] = {0, 0, 0};
  const int32_t* origin_ptr = origin;
  int dummy = 0;
  const void* ptrs[2] = {&dummy, &dummy};
};

int line(const char* subject, const slf_module_desc& d, const Call& call) {
  slf::ModuleConfig c;
  const char* why = "";
  if (slf::module_config(&d, &c, &why)) {
    printf("%s\t-1\tmodule_config: %s\n", subject, why);
    return 1;
  }
  static const char* const names[2] = {"pos", "acc"};
  std::string err;
  const int rc = slf::ibm_check(c, call.has_field, "slf_ibm_test", call.n, call.origin_ptr, call.ptrs, names, 2, &err);
  printf("%s\t%d\t%s\n", subject, rc, err.c_str());
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += line("served-d2q9", base_desc(SLF_D2Q9), Call());
  {
    slf_module_desc d = base_desc(SLF_D3Q19);
    d.precision = 8; d.model = SLF_MRT; d.access_pattern = SLF_AA;
    Call c; c.n = 1; c.origin[0] = -5; c.origin[2] = 1 << 30;
    bad += line("served-d3q19-f64", d, c);
  }
  { slf_module_desc d = base_desc(SLF_D3Q19); d.accel_field = 0; bad += line("no-accel-field", d, Call()); }
  { Call c; c.has_field = false; bad += line("field-not-set", base_desc(SLF_D3Q19), c); }
  { Call c; c.n = 0; bad += line("zero-markers", base_desc(SLF_D3Q19), c); }
  { Call c; c.n = -7; bad += line("negative-markers", base_desc(SLF_D3Q19), c); }
  { Call c; c.n = (1 << 24) + 1; bad += line("too-many-markers", base_desc(SLF_D3Q19), c); }
  { Call c; c.origin_ptr = nullptr; bad += line("null-origin", base_desc(SLF_D3Q19), c); }
  { Call c; c.origin[1] = (1 << 30) + 1; bad += line("origin-out-of-range", base_desc(SLF_D3Q19), c); }
  { Call c; c.ptrs[0] = nullptr; bad += line("null-pos", base_desc(SLF_D2Q9), c); }
  { Call c; c.ptrs[1] = nullptr; bad += line("null-acc", base_desc(SLF_D2Q9), c); }
  bad += line("d3q15", base_desc(SLF_D3Q15), Call());
  bad += line("d3q27", base_desc(SLF_D3Q27), Call());
  return bad ? 2 : 0;
}
