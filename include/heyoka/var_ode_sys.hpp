// Drop-in include path of the reference (include/heyoka/var_ode_sys.hpp): forwards to the MI355X-native implementation
// under heyoka_amd/csrc/ and exposes it as namespace heyoka, so that sources written against the reference's headers
// compile unchanged with -I <repo>/include -lheyoka_amd.
#pragma once
#include "../../heyoka_amd/csrc/var_ode_sys.hpp"
#include "../../heyoka_amd/csrc/expression_diff.hpp"

#ifndef HEYOKA_AMD_NAMESPACE_ALIAS
#define HEYOKA_AMD_NAMESPACE_ALIAS
namespace heyoka = heyoka_amd;
#endif
