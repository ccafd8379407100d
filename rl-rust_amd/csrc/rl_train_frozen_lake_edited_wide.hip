// rl_train_frozen_lake_edited_wide.hip — kernel instantiations for ENV_FLE_WIDE: FrozenLakeEditedEnv on a
// wide map (rl_map_register_wide); see rl_train_frozen_lake_wide.hip.
#include "rl_train_impl.h"

namespace rlamd {
train_launch_fn train_table_frozen_lake_edited_wide(int agent, int policy, int sel, int algo, int priv) {
    return train_table_entry<ENV_FLE_WIDE>(agent, policy, sel, algo, priv);
}
}  // namespace rlamd
