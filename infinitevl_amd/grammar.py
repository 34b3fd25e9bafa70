"""Token-level finite state machines for constrained decoding: the host side (numpy only, no device work).

A `TokenFsm` says, per state, which tokens a stream may emit and where each of them leads.  The sampling launch
(ivl_sample_rows_fwd in include/ivl_hip.h) reads its compact tables on the device: the allowed-token bitmap of the row's
state restricts the draw, and the emitted token advances the state, with no host round trip per token.  This is what HF
generate's `prefix_allowed_tokens_fn` serves (INTEGRATION.md maps one onto the other).

Three builders: `from_edges` (explicit transitions), `from_choices` (a closed set of token sequences: labels, tool names, a
forced prefix) and `from_byte_dfa` (a byte-level DFA that someone else compiled from a regex or a schema, lifted to the
tokens of a vocabulary).  Each derives
  * token classes: tokens whose column over all states is identical share a class (numbered by their lowest token id), so the
    transition table is [n_states, n_classes], not [n_states, V];
  * mask uint32 [n_states, ceil(V/32)] (bit (i & 31) of word (i >> 5) of row q = token i is allowed in state q),
    cls int32 [V] and trans int32 [n_states, n_classes] (a state >= 0, FREE = -1: the row becomes unconstrained, NONE = -2: no
    transition).  Mask and transitions are consistent by construction: bit set <=> transition != NONE.
`allowed` and `step` are the host reference of what the kernel does with the tables.
"""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import numpy as np


class TokenFsm:
    FREE = -1          # as a next state: the row becomes unconstrained; as `then` of from_choices: the same after a choice
    NONE = -2          # no transition
    END = -3           # `then` of from_choices: after a complete choice only the stop ids are allowed

    def __init__(self, nxt: np.ndarray, start: int = 0):
        """nxt: int32 [n_states, V], the next state of every (state, token): >= 0, FREE or NONE.  (The builders make it.)"""
        nxt = np.ascontiguousarray(nxt, dtype=np.int32)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1:
            raise ValueError(f"TokenFsm: the transitions must be [n_states >= 1, vocab_size >= 1]; got {nxt.shape}")
        n, V = nxt.shape
        if ((nxt < self.NONE) | (nxt >= n)).any():
            raise ValueError(f"TokenFsm: a next state outside [0, {n}), FREE and NONE")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < n:
            raise ValueError(f"TokenFsm: start must be a state in [0, {n}); got {start!r}")
        self.n_states, self.vocab_size, self.start = n, V, int(start)
        # classes: the distinct columns, numbered by the lowest token id that has them
        _, first, inv = np.unique(nxt.T, axis=0, return_index=True, return_inverse=True)
        rank = np.empty(first.shape[0], dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])
        self.cls = rank[inv.reshape(-1)].astype(np.int32)
        self.n_classes = int(first.shape[0])
        self.trans = np.ascontiguousarray(nxt[:, np.sort(first)], dtype=np.int32)
        words = (V + 31) // 32
        bits = np.zeros((n, words * 32), dtype=bool)
        bits[:, :V] = nxt != self.NONE
        self.mask = np.packbits(bits.reshape(n, -1, 8), axis=2, bitorder="little").reshape(n, -1).view("<u4").copy()
        self._check_reachable()

    def _check_reachable(self) -> None:
        seen, todo = {self.start}, [self.start]
        while todo:
            q = todo.pop()
            row = self.trans[q]
            if not (row != self.NONE).any():
                raise ValueError(f"TokenFsm: state {q} is reachable from the start state {self.start} and allows no token")
            for t in np.unique(row[row >= 0]).tolist():
                if t not in seen:
                    seen.add(t)
                    todo.append(t)

    # ---- the host reference ------------------------------------------------------------------------------------------------
    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens a row in `state` may emit (everything for FREE)."""
        if state == self.FREE:
            return np.ones(self.vocab_size, dtype=bool)
        return self.trans[self._state(state)][self.cls] != self.NONE

    def step(self, state: int, token: int) -> int:
        """The state after `token` was emitted in `state`: >= 0 or FREE (FREE stays FREE).  A token the state does not allow is
        a ValueError."""
        if not 0 <= int(token) < self.vocab_size:
            raise ValueError(f"TokenFsm.step: token {token!r} outside [0, {self.vocab_size})")
        if state == self.FREE:
            return self.FREE
        nxt = int(self.trans[self._state(state), self.cls[int(token)]])
        if nxt == self.NONE:
            raise ValueError(f"TokenFsm.step: state {state} does not allow token {token}")
        return nxt

    def _state(self, state) -> int:
        if isinstance(state, bool) or not isinstance(state, (int, np.integer)) or not 0 <= state < self.n_states:
            raise ValueError(f"TokenFsm: state must be FREE or in [0, {self.n_states}); got {state!r}")
        return int(state)

    # ---- builders ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _vocab(who: str, vocab_size) -> int:
        if isinstance(vocab_size, bool) or not isinstance(vocab_size, (int, np.integer)) or vocab_size < 1:
            raise ValueError(f"{who}: vocab_size must be an int >= 1; got {vocab_size!r}")
        return int(vocab_size)

    @staticmethod
    def _ids(who: str, what: str, ids: Iterable[int], V: int) -> List[int]:
        ids = [ids] if isinstance(ids, (int, np.integer)) and not isinstance(ids, bool) else list(ids)
        if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t < V for t in ids):
            raise ValueError(f"{who}: {what} must be token ids in [0, {V}); got {ids!r}")
        return [int(t) for t in ids]

    @classmethod
    def from_edges(cls, vocab_size: int, n_states: int, edges: Sequence[Tuple[int, Iterable[int], int]], start: int = 0) -> "TokenFsm":
        """edges: (state, token_ids, next_state) triples; next_state may be TokenFsm.FREE.  Every (state, token) not named has
        no transition.  Naming one twice with different targets is a ValueError."""
        who = "TokenFsm.from_edges"
        V = cls._vocab(who, vocab_size)
        if isinstance(n_states, bool) or not isinstance(n_states, (int, np.integer)) or n_states < 1:
            raise ValueError(f"{who}: n_states must be an int >= 1; got {n_states!r}")
        nxt = np.full((n_states, V), cls.NONE, dtype=np.int32)
        for q, ids, to in edges:
            if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= q < n_states:
                raise ValueError(f"{who}: state {q!r} outside [0, {n_states})")
            if isinstance(to, bool) or not isinstance(to, (int, np.integer)) or not (to == cls.FREE or 0 <= to < n_states):
                raise ValueError(f"{who}: next state {to!r} is neither FREE nor in [0, {n_states})")
            ids = np.asarray(cls._ids(who, "token_ids", ids, V), dtype=np.int64)
            was = nxt[q, ids]
            if ((was != cls.NONE) & (was != to)).any():
                raise ValueError(f"{who}: state {q} has two targets for token {int(ids[(was != cls.NONE) & (was != to)][0])}")
            nxt[q, ids] = to
        return cls(nxt, start)

    @classmethod
    def from_choices(cls, vocab_size: int, choices: Sequence[Sequence[int]], stop_token_ids: Iterable[int] = (),
                     then: int = END) -> "TokenFsm":
        """A trie over the token-id sequences `choices` (each non-empty; choices that are prefixes of each other are legal).
        then = TokenFsm.END: after a complete choice only the stop ids are allowed (and keep being allowed: the row ends through
        the sampler's stop rule); a choice that is a prefix of another allows the stop ids beside the continuation.
        then = TokenFsm.FREE: the row becomes unconstrained with the last token of the shortest complete choice on its path."""
        who = "TokenFsm.from_choices"
        V = cls._vocab(who, vocab_size)
        if then not in (cls.END, cls.FREE):
            raise ValueError(f"{who}: then must be TokenFsm.END or TokenFsm.FREE; got {then!r}")
        stop = cls._ids(who, "stop_token_ids", stop_token_ids, V)
        seqs = [cls._ids(who, "a choice", c, V) for c in choices]
        if not seqs or any(not s for s in seqs):
            raise ValueError(f"{who}: at least one choice, none of them empty")
        if then == cls.END and not stop:
            raise ValueError(f"{who}: then = END needs stop_token_ids (nothing else is allowed after a complete choice)")
        kids: List[dict] = [{}]                          # node -> {token: node}
        complete = [False]
        for s in seqs:
            q = 0
            for t in s:
                if t not in kids[q]:
                    kids[q][t] = len(kids)
                    kids.append({})
                    complete.append(False)
                q = kids[q][t]
            complete[q] = True
        # states: the trie nodes that are not complete leaves (under FREE: that are not complete), then the end state
        keep = [q for q in range(len(kids)) if not complete[q] or (then == cls.END and kids[q])]
        index = {q: i for i, q in enumerate(keep)}
        end = len(keep) if then == cls.END else None
        nxt = np.full((len(keep) + (then == cls.END), V), cls.NONE, dtype=np.int32)
        for q in keep:
            for t, c in kids[q].items():
                nxt[index[q], t] = index[c] if c in index else (end if then == cls.END else cls.FREE)
            if complete[q]:                              # (END only) a choice that is a prefix of another: it may stop here
                nxt[index[q], stop] = end
        if then == cls.END:
            nxt[end, stop] = end
        return cls(nxt, 0)

    @classmethod
    def from_byte_dfa(cls, vocab: Sequence[bytes], byte_trans, start: int, accepting: Iterable[int],
                      stop_token_ids: Iterable[int] = ()) -> "TokenFsm":
        """Lifts a byte-level DFA to tokens.  vocab: one `bytes` per token id (an empty entry is never allowed); byte_trans:
        int32 [n, 256], -1 = no transition.  Token t is allowed in state q iff walking its bytes from q never leaves the DFA,
        and leads to where the walk ends.  The stop ids are allowed exactly in the accepting states (whatever their bytes);
        they lead to one further state, n, which allows only them."""
        who = "TokenFsm.from_byte_dfa"
        bt = np.asarray(byte_trans)
        if bt.ndim != 2 or bt.shape[1] != 256 or bt.shape[0] < 1 or not np.issubdtype(bt.dtype, np.integer):
            raise ValueError(f"{who}: byte_trans must be an integer array [n >= 1, 256]; got {bt.dtype} {bt.shape}")
        n = bt.shape[0]
        if ((bt < -1) | (bt >= n)).any():
            raise ValueError(f"{who}: byte_trans holds a state outside [0, {n}) and -1")
        V = cls._vocab(who, len(vocab))
        if any(not isinstance(b, (bytes, bytearray)) for b in vocab):
            raise ValueError(f"{who}: vocab must hold one bytes object per token id")
        stop = cls._ids(who, "stop_token_ids", stop_token_ids, V)
        acc = cls._ids(who, "accepting", accepting, n)
        lens = np.fromiter((len(b) for b in vocab), dtype=np.int64, count=V)
        flat = np.frombuffer(b"".join(bytes(b) for b in vocab), dtype=np.uint8)
        begin = np.concatenate([[0], np.cumsum(lens)[:-1]])
        # every state x every token at once: column t walks vocab[t]; a dead walk stays dead (row n of `table`)
        table = np.concatenate([bt.astype(np.int32), np.full((1, 256), -1, dtype=np.int32)])
        cur = np.repeat(np.arange(n, dtype=np.int32)[:, None], V, axis=1)
        for pos in range(int(lens.max()) if V else 0):
            live = np.nonzero(lens > pos)[0]
            byte = flat[begin[live] + pos]
            c = cur[:, live]
            cur[:, live] = table[np.where(c < 0, n, c), byte[None, :]]
        nxt = np.where(cur < 0, cls.NONE, cur).astype(np.int32)
        nxt[:, lens == 0] = cls.NONE
        if stop:
            nxt = np.concatenate([nxt, np.full((1, V), cls.NONE, dtype=np.int32)])
            nxt[:, stop] = cls.NONE
            nxt[np.asarray(acc + [n], dtype=np.int64)[:, None], np.asarray(stop, dtype=np.int64)[None, :]] = n
        return cls(nxt, start)
