// fsk_load_plan.hip — the library's translation unit for the load plan. The plan itself is fsk_load_plan.cpp, plain C++
// that a host-only program can link (tests/host/load_plan_check.cpp does); every build of the library — the product and
// the CPU emulation alike — takes its units from the .hip files of this directory, so the plan joins them through this one.
#include "fsk_load_plan.cpp"
