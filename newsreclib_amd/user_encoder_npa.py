"""Mirror of the reference's NPA ``UserEncoder`` (components/encoders/user/npa.py): same constructor, attributes and
``state_dict`` keys.  The news query comes from ``ops_npa.NpaUserQueriesFn`` (with the text queries, in one launch);
this module runs the personalized attention over the ragged history rows."""
from __future__ import annotations

import torch
import torch.nn as nn

from .npa_layers import PersonalizedAttention, UserPreferenceQueryProjection
from .ops_npa import PersonalizedUserAttentionFn


class UserEncoder(nn.Module):
    def __init__(self, user_embed_dim: int, num_filters: int, preference_query_dim: int,
                 dropout_probability: float) -> None:
        super().__init__()
        self.news_query_projection = UserPreferenceQueryProjection(
            user_embed_dim=user_embed_dim, preference_query_dim=preference_query_dim,
            dropout_probability=dropout_probability)
        self.personalized_attention = PersonalizedAttention(preference_query_dim=preference_query_dim,
                                                            num_filters=num_filters)

    def forward(self, hist_news_vector: torch.Tensor, hist_offsets: torch.Tensor, max_hist: int,
                news_queries: torch.Tensor) -> torch.Tensor:
        """hist_news_vector (n_hist, F) ragged rows, hist_offsets (B + 1), news_queries (B, F) = the tanh'd queries.
        Each user's softmax also counts ``max_hist - n_b`` zero rows, as the reference's ``to_dense_batch`` input
        (user/npa.py:58-60)."""
        return PersonalizedUserAttentionFn.apply(hist_news_vector, hist_offsets, max_hist, news_queries)
