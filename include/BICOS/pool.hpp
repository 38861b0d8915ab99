// BICOS/pool.hpp -- the installed name of <bicos/pool.hpp>: BICOS::pool_stack and
// BICOS::match_pyramid, the coarse-to-fine match over the guided BICOS::match overload
// (<bicos/match.hpp>, <bicos/guide.hpp>). An extension: the reference has no counterpart.
#pragma once

#include "../bicos/guide.hpp"
#include "../bicos/match.hpp"
#include "../bicos/pool.hpp"
