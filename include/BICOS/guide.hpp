// BICOS/guide.hpp -- the installed name of <bicos/guide.hpp>: BICOS::guide_from_disparity, the
// builder of the per-pixel disparity windows that the guided BICOS::match overload
// (<bicos/match.hpp>) takes. An extension: the reference has no counterpart.
#pragma once

#include "../bicos/guide.hpp"
#include "../bicos/match.hpp"
