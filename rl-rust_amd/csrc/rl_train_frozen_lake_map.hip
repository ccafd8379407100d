// rl_train_frozen_lake_map.hip — kernel instantiations for ENV_FL_MAP: FrozenLakeEnv on a registered
// map (rl_map_register), whose reset lands on the map's own start cells (rl_device.h EnvDevMap).  A
// translation unit of its own, so the built-in maps' instantiations are untouched by it.
#include "rl_train_impl.h"

namespace rlamd {
train_launch_fn train_table_frozen_lake_map(int agent, int policy, int sel, int algo, int priv) {
    return train_table_entry<ENV_FL_MAP>(agent, policy, sel, algo, priv);
}
}  // namespace rlamd
