// ses_env_blobs.h -- the state blobs of the step-wise envs that ses_envs.hip owns, for the units that read them (ses_envs.hip
// steps them, ses_render.hip draws them).  Opaque to callers, fixed per handle: CartPole {x, xd, th, thd}; simple_spread
// SpreadState<NA> + the cycle counter; BipedalWalker the env struct of the Box2D-style world followed by the episode's terrain
// heights (LunarLander's LanderBlob is in ses_lander.h, beside the discrete lander that shares it).
#pragma once
#include "ses_cartpole.h"
#include "ses_lander.h"
#include "ses_spread.h"
#include "ses_walker.h"

namespace ses {

struct CartPoleBlob {
    CartPoleState st;
};

template <int NA>
struct SpreadBlob {
    SpreadState<NA> st;
    int32_t cycle;
};

struct WalkerBlob {
    b2l::WalkerEnv env;
    float ty[BW_TERRAIN_ROW];
};

}  // namespace ses
