"""Parameter-holding mirrors of the reference's NPA layers (components/layers/projection.py:8-98,
attention.py:212-259): same constructor signatures, attribute names and ``state_dict`` keys.  Their arithmetic runs
fused in the HIP kernels of ``ops_npa`` (``NpaUserQueriesFn`` for both projections and the query side of
``PersonalizedAttention``; ``NpaEncoderFn`` / ``PersonalizedUserAttentionFn`` for the pooling), so none of them has a
``forward`` of its own."""
from __future__ import annotations

import torch
import torch.nn as nn


class UserProjection(nn.Module):
    """``user_embed`` (num_users, user_embed_dim), initialised with ``torch.rand`` as the reference (projection.py:40)."""

    def __init__(self, num_users: int, user_embed_dim: int, dropout_probability: float) -> None:
        super().__init__()
        if not isinstance(num_users, int):
            raise ValueError(f"Expected keyword argument `num_users` to be an `int` but got {num_users}")
        if not isinstance(user_embed_dim, int):
            raise ValueError(f"Expected keyword argument `user_embed_dim` to be an `int` but got {user_embed_dim}")
        if not isinstance(dropout_probability, float):
            raise ValueError(
                f"Expected keyword argument `dropout_probability` to be a `float` but got {dropout_probability}")
        self.user_embed = nn.Parameter(torch.rand(num_users, user_embed_dim))
        self.dropout = nn.Dropout(p=dropout_probability)


class UserPreferenceQueryProjection(nn.Module):
    """``dropout(relu(preference_query_projection(u)))`` (projection.py:85-98)."""

    def __init__(self, user_embed_dim: int, preference_query_dim: int, dropout_probability: float) -> None:
        super().__init__()
        if not isinstance(user_embed_dim, int):
            raise ValueError(f"Expected keyword argument `user_embed_dim` to be an `int` but got {user_embed_dim}")
        if not isinstance(preference_query_dim, int):
            raise ValueError(
                f"Expected keyword argument `preference_query_dim` to be an `int` but got {preference_query_dim}")
        if not isinstance(dropout_probability, float):
            raise ValueError(
                f"Expected keyword argument `dropout_probability` to be a `float` but got {dropout_probability}")
        self.preference_query_projection = nn.Linear(user_embed_dim, preference_query_dim)
        self.dropout = nn.Dropout(p=dropout_probability)


class PersonalizedAttention(nn.Module):
    """``softmax(tanh(preference_query_projection(q)) . keys)``-weighted sum of the keys (attention.py:244-259)."""

    def __init__(self, preference_query_dim: int, num_filters: int) -> None:
        super().__init__()
        if not isinstance(preference_query_dim, int):
            raise ValueError(
                f"Expected keyword argument `preference_query_dim` to be an `int` but got {preference_query_dim}")
        if not isinstance(num_filters, int):
            raise ValueError(f"Expected keyword argument `num_filters` to be an `int` but got {num_filters}")
        self.preference_query_projection = nn.Linear(preference_query_dim, num_filters)


def query_head(projection: UserPreferenceQueryProjection, attention: PersonalizedAttention):
    """The four tensors of one query head, in the order ``ops_npa.NpaUserQueriesFn`` takes them."""
    return (projection.preference_query_projection.weight, projection.preference_query_projection.bias,
            attention.preference_query_projection.weight, attention.preference_query_projection.bias)
