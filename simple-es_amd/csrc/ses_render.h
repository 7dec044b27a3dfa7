// ses_render.h -- what the renderer's two layers agree on (ses_render.hip): the primitive record, the
// palette, and the constants of the four scenes.  A frame is width x height palette indices (one byte a pixel, row 0 on top);
// a scene builder turns one env state blob into at most SES_RENDER_MAX_PRIMS integer primitives, the rasteriser turns F such
// lists into F frames.  include/ses.h states the primitive contract for callers; this header is the unit's own copy of the
// numbers plus everything a scene needs.
#pragma once
#include <stdint.h>

namespace ses {

// int32[8] = {kind, colour, x0, y0, x1, y1, x2, y2}; coordinates in 1/16 pixel, origin top-left, y down
constexpr int RENDER_WORDS = 8;
constexpr int RENDER_MAX_PRIMS = 256;            // SES_RENDER_MAX_PRIMS
constexpr int RENDER_MAX_SIDE = 1024;            // frames of up to 1024 x 1024
constexpr int RENDER_COORD_MIN = -16384, RENDER_COORD_MAX = 16383;
constexpr int RENDER_TRI = 0, RENDER_DISC = 1, RENDER_CAPSULE = 2, RENDER_FILL = 3;

// the palette (ses_render_palette; ses/render.py carries the same 48 bytes)
constexpr int PAL_BLACK = 0, PAL_WHITE = 1, PAL_SKY = 2, PAL_GRASS = 3, PAL_RED = 4, PAL_YELLOW = 5, PAL_HULL = 6, PAL_LANDER_LEG = 7,
              PAL_POLE = 8, PAL_AXLE = 9, PAL_LEG_NEAR = 10, PAL_LEG_FAR = 11, PAL_LANDMARK = 12, PAL_AGENT = 13, PAL_GREY = 14,
              PAL_FLAG = 15;
constexpr uint8_t RENDER_PALETTE[48] = {
    0,   0,   0,      // 0  black: CartPole's cart and track, the walker's flag pole, LunarLander's sky
    255, 255, 255,    // 1  white: CartPole's and simple_spread's background, the moon, the helipad poles
    230, 230, 255,    // 2  sky: BipedalWalker's background
    102, 153, 76,     // 3  grass: BipedalWalker's terrain
    255, 0,   0,      // 4  red: the lidar rays
    204, 204, 0,      // 5  yellow: the helipad flags
    127, 102, 230,    // 6  hull: the lander's and the walker's hull
    77,  77,  128,    // 7  the lander's legs
    204, 153, 102,    // 8  CartPole's pole
    127, 127, 204,    // 9  CartPole's axle
    178, 102, 153,    // 10 the walker's leg -1 (bodies 1, 2)
    127, 51,  102,    // 11 the walker's leg +1 (bodies 3, 4)
    64,  64,  64,     // 12 simple_spread's landmarks
    89,  89,  217,    // 13 simple_spread's agents
    128, 128, 128,    // 14 grey (no scene uses it)
    230, 51,  0,      // 15 the walker's start flag
};

// ---- the scenes' canvases and constants (pixels; 16 units a pixel) ----------------------------------------------------------
constexpr int CP_W = 600, CP_H = 400;
constexpr float CP_PX_PER_UNIT = 125.0f, CP_CENTRE_X = 300.0f, CP_CART_Y = 100.0f, CP_CART_HALF_W = 25.0f, CP_CART_HALF_H = 15.0f,
                CP_PIVOT_Y = 107.5f, CP_POLE_LEN = 120.0f;
constexpr int CP_TRACK_R = 8, CP_POLE_R = 80, CP_AXLE_R = 80;                  // units

constexpr int BOX2D_W = 600, BOX2D_H = 400;                                      // LunarLander and BipedalWalker
constexpr float BOX2D_PX_PER_UNIT = 30.0f;
constexpr float LL_FLAG_POLE = 50.0f / 30.0f, LL_FLAG_DROP = 10.0f / 30.0f, LL_FLAG_MID = 5.0f / 30.0f, LL_FLAG_LEN = 25.0f / 30.0f;
constexpr float LL_HELIPAD_X1 = 8.0f, LL_HELIPAD_X2 = 12.0f;                    // terrain points 4 and 6
constexpr int LL_POLE_R = 8;                                                     // units
constexpr float BW_SCROLL_LEAD = 600.0f / 30.0f / 5.0f;                         // scroll = hull x - this
constexpr int BW_LIDAR_R = 8, BW_FLAG_POLE_R = 16;                               // units

constexpr int SP_W = 400, SP_H = 400;
constexpr float SP_PX_PER_UNIT = 100.0f, SP_CENTRE = 200.0f;
constexpr int SP_LANDMARK_R = 80, SP_AGENT_R = 240;                              // 0.05 and 0.15 world units

// Reacher: the plane seen from above, the shoulder in the middle of a 400 x 400 canvas, 500 px per metre (the arm reaches 105 px,
// the target square 135 px).  The scene is computed in float64 from the float64 state with the env's own sincos_ieee.
constexpr int RC_W = 400, RC_H = 400;
constexpr double RC_PX_PER_UNIT = 500.0, RC_CENTRE = 200.0;
constexpr int RC_LINK_R = 56, RC_TIP_R = 80, RC_TARGET_R = 96;                   // units: 3.5, 5 and 6 px

}  // namespace ses
