// step_action: an MI355X extension with no counterpart in the reference (a step callback defined by expressions and applied on
// the device), kept next to callback/angle_reducer.hpp so that sources written against <heyoka/...> find it: forwards to
// the implementation under heyoka_amd/csrc/ and exposes it as namespace heyoka.
#pragma once
#include "../../../heyoka_amd/csrc/step_action.hpp"

#ifndef HEYOKA_AMD_NAMESPACE_ALIAS
#define HEYOKA_AMD_NAMESPACE_ALIAS
namespace heyoka = heyoka_amd;
#endif
