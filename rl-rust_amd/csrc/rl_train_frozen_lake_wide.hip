// rl_train_frozen_lake_wide.hip — kernel instantiations for ENV_FL_WIDE: FrozenLakeEnv on a wide map
// (rl_map_register_wide, up to 1024 cells), stepped over the u16 (state, direction) table (rl_device.h
// EnvDevWide).  A translation unit of its own, so the other maps' instantiations are untouched by it.
#include "rl_train_impl.h"

namespace rlamd {
train_launch_fn train_table_frozen_lake_wide(int agent, int policy, int sel, int algo, int priv) {
    return train_table_entry<ENV_FL_WIDE>(agent, policy, sel, algo, priv);
}
}  // namespace rlamd
