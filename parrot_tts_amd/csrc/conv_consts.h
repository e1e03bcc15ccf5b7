// conv_consts.h -- the conv plan's mode constants and the size of the tile table (conv_mfma.h): what host code that launches no
// conv kernel itself needs of them.
#pragma once
namespace parrot {
enum { PRE_NONE = 0, PRE_LRELU = 1 };
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };
enum { EPI_STORE = 0, EPI_ADD = 1, EPI_ADD_DIV = 2 };

constexpr int NUM_TILE_CFGS = 7;  // tile table of conv_mfma.h (index = parrot_conv_desc.tile_cfg)
}  // namespace parrot
