"""YouTubeRec (the reference's tf1/recommenders/youtube_rec.py with tf1/modules/interactions/mlp_softmax.py and
tf1/modules/extractions/multi_layer_fc.py): VanillaYouTubeRec with categorical user features.  Each feature has an embedding
table; the looked-up rows are concatenated in front of the pooled history, the result goes through Dense + bias + relu, and the
output meets the item table in a softmax over all items (rt.DeepSeqRec),
    x0 = [ S_1[f_1] | ... | S_m[f_m] | pool(H[seq_item_id[:seq_len]]) ];   x_{l+1} = relu(x_l W_l + c_l);   s(q, i) = x_L . V[i] (+ b[i]).
The arguments are the reference's dicts: user_dict {feature: number of values} -- its order is the order of the columns, the
reference's being gender, geo --, item_dict {'id': total_items}, dim_user_embed {feature: dim, ..., 'total': their sum},
dim_item_embed {'id': dim, 'total': dim}.  hidden=None is the reference's architecture: ONE layer of width
dim_user_embed['total'] + dim_item_embed['total'] whose output is scored against an item table of that width (the reference's
Dense(total_items) kernel).  Deviations: no dropout; embeddings take LatentFactor's default initializer, the layers Xavier-uniform
weights and zero biases; l2_reg_embed sits on x0 (the looked-up feature rows and the POOLED vector) and on the labels' item rows;
training is `train_steps_full` (the sampled-negatives form with a tower is not offered)."""
from .vanilla_youtube_rec import VanillaYouTubeRec


class YouTubeRec(VanillaYouTubeRec):

    def __init__(self, user_dict, item_dict, dim_user_embed, dim_item_embed, max_seq_len, l2_reg_embed=None, l2_reg_mlp=None,
                 hidden=None, use_item_bias=False, pool=None, ctx=None):
        what = "YouTubeRec"
        names = list(user_dict)
        missing = [k for k in names if k not in dim_user_embed]
        if missing or "id" not in item_dict or "id" not in dim_item_embed:
            raise ValueError(f"{what}: dim_user_embed lacks {missing}" if missing else f"{what}: item_dict and dim_item_embed need the key 'id'")
        if len(names) > 4:
            raise ValueError(f"{what}: {len(names)} user features; at most 4")
        side = tuple((k, int(user_dict[k]), int(dim_user_embed[k])) for k in names)
        du, di = sum(d for _, _, d in side), int(dim_item_embed["id"])
        if int(dim_user_embed.get("total", du)) != du or int(dim_item_embed.get("total", di)) != di:
            raise ValueError(f"{what}: a 'total' that is not the sum of its dims (user {du}, item {di})")
        if hidden is None:
            hidden = [du + di]
        self._build(what, di, max_seq_len, int(item_dict["id"]), l2_reg_embed, l2_reg_mlp, use_item_bias, pool, ctx, hidden, side)
