// rl_train_frozen_lake_edited_map.hip — kernel instantiations for ENV_FLE_MAP: FrozenLakeEditedEnv on a
// registered map (rl_map_register); see rl_train_frozen_lake_map.hip.
#include "rl_train_impl.h"

namespace rlamd {
train_launch_fn train_table_frozen_lake_edited_map(int agent, int policy, int sel, int algo, int priv) {
    return train_table_entry<ENV_FLE_MAP>(agent, policy, sel, algo, priv);
}
}  // namespace rlamd
