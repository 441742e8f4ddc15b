"""MultDAE (Liang et al. 2018, "Variational Autoencoders for Collaborative Filtering", the denoising autoencoder with the
multinomial likelihood): a user's bag of items is encoded and decoded into logits over ALL items, and the loss is the multinomial
log-likelihood of the user's whole item set,
    x0 = pool(H[in_items]);   x_{l+1} = relu(x_l W_l + c_l);   s(q, i) = x_L . V[i] + b[i];   l = -sum_{e in set} log softmax(s)[j_e].
The encoder's first layer over the multi-hot input is the pooled history table H (a bag pool IS a multi-hot row times a matrix),
the hidden layers are the tower's, the decoder is the item table V with its bias: VanillaYouTubeRec with `train_steps_sets` as
its training step.  The dropout on the input happens in the data (data.autoencoder_batches drops entries of the input bag), so
no dropout runs on the device.  Deviations from the paper: relu where it has tanh; pool "mean" (or "sum" / ("fixed", denom))
where it divides by sqrt(len); no VAE sampling or KL term (this is Mult-DAE, not Mult-VAE); the last layer has a relu when
hidden layers are given, as the parent's tower has.  `inference`, `recommend`, `score` and `evaluate` take histories and are
the parent's: a user never trained on is served from a fold-in history alone."""
from .vanilla_youtube_rec import VanillaYouTubeRec

_ANY_LEN = 2 ** 31 - 1          # (no max_seq_len: a bag is as long as the user's list)


class MultDAE(VanillaYouTubeRec):

    def __init__(self, dim_embed, total_items, hidden=None, l2_reg_embed=None, l2_reg_mlp=None, use_item_bias=True, pool="mean",
                 ctx=None):
        """dim_embed: the width of the encoder's first layer (the history table's dim); hidden: None -- the pooled vector meets
        the decoder directly --, or the widths of 1 .. 4 further Dense + bias + relu layers, the last one the decoder's dim."""
        self._build("MultDAE", dim_embed, _ANY_LEN, total_items, l2_reg_embed, l2_reg_mlp, use_item_bias, pool, ctx, hidden, ())

    def train_steps(self, optimizer, in_items, in_len, label_items, label_len, label_weight=None, sample_weight=None,
                    item_offset=None, want_loss=True, train=None):
        """One train step in one device call: input bags in_items [B, L] of which in_len [B] entries count, label sets
        label_items [B, Ll] / label_len [B] (data.autoencoder_batches makes both).  -> (loss[1], l2[1]) when want_loss"""
        return self.train_steps_sets(optimizer, in_items, in_len, label_items, label_len, label_weight=label_weight,
                                     sample_weight=sample_weight, item_offset=item_offset, want_loss=want_loss, train=train)

    def loss(self, in_items, in_len, label_items, label_len, label_weight=None, sample_weight=None, item_offset=None):
        """the forward of train_steps alone -> (loss, l2)"""
        return self.loss_sets(in_items, in_len, label_items, label_len, label_weight=label_weight, sample_weight=sample_weight,
                              item_offset=item_offset)
