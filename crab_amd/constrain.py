"""Closed-set generation: the answer sets of an evaluation (MUSIC-AVQA's answer vocabulary, AVE's 28 event labels, AVVP's label list) as a token
trie that the decode step walks ON THE DEVICE (csrc/constrain.hip, crab_constrained_select).

A Hugging Face user constrains a decode with `prefix_allowed_tokens_fn`, a Python callback between two tokens.  GenerationEngine's decode step is one
captured HIP graph whose step, position and finished flags live in device memory: no host code runs between two tokens, so the callback is refused by
name (UnifiedForCausalLM._UNSUPPORTED) and this module is what replaces it.  TokenTrie.allowed() is exactly what such a callback would return.

Layout: one forest for all sets, one root per set, flattened to CSR int32 arrays -
    edge_off [n_nodes + 1], edge_tok [n_edges], edge_dst [n_edges], roots [n_sets]
node n owns the edges edge_off[n] .. edge_off[n + 1] - 1, sorted by ascending token id.  A node that ends a sequence is terminal: its EOS edge is
materialised here, in sorted position, and leads to ONE shared sink node without edges - the kernel sees only edges.  A sequence that is a proper
prefix of another keeps both its children and the EOS edge; duplicates within a set merge.  With a closed set every output (cut at EOS) is a member
by construction, and a row ends after the few tokens of its answer plus EOS.  When max_new_tokens runs out in the middle of an answer the row holds
a proper prefix of a member, as HF's constrained decode does."""
from typing import List, Optional, Sequence

import numpy as np


class TokenTrie:
    def __init__(self, sets, vocab_size: int, eos_token_id: Optional[int], min_new_tokens: int = 0):
        if eos_token_id is None:
            raise ValueError("TokenTrie: eos_token_id is None - constrained generation needs ONE EOS id (a closed-set answer ends by emitting it; "
                             "HF's own constrained decode has no defined end without one)")
        if isinstance(eos_token_id, (list, tuple)):
            if len(set(int(e) for e in eos_token_id)) != 1:
                raise ValueError(f"TokenTrie: eos_token_id = {list(eos_token_id)}: constrained generation needs ONE EOS id")
            eos_token_id = eos_token_id[0]
        V, eos = int(vocab_size), int(eos_token_id)
        if not 0 <= eos < V:
            raise ValueError(f"TokenTrie: eos_token_id {eos} is outside the vocabulary [0, {V})")
        sets = [list(s) for s in sets]
        if not sets:
            raise ValueError("TokenTrie: no answer set")
        children = [{}]                                       # node -> {token: node}; node 0 is the shared sink
        terminal = [False]
        roots, min_len = [], None
        for si, seqs in enumerate(sets):
            if not seqs:
                raise ValueError(f"TokenTrie: answer set {si} is empty")
            root = len(children)
            children.append({}); terminal.append(False)
            roots.append(root)
            for seq in seqs:
                seq = [int(t) for t in seq]
                if not seq:
                    raise ValueError(f"TokenTrie: answer set {si} holds an empty sequence")
                n = root
                for t in seq:
                    if not 0 <= t < V:
                        raise ValueError(f"TokenTrie: token id {t} of answer set {si} is outside the vocabulary [0, {V})")
                    if t == eos:
                        raise ValueError(f"TokenTrie: a sequence of answer set {si} contains the EOS id {eos} (EOS ends an answer, the trie adds it)")
                    nxt = children[n].get(t)
                    if nxt is None:
                        nxt = len(children)
                        children.append({}); terminal.append(False)
                        children[n][t] = nxt
                    n = nxt
                terminal[n] = True
                min_len = len(seq) if min_len is None else min(min_len, len(seq))
        edge_off, edge_tok, edge_dst = [0], [], []
        for n, ch in enumerate(children):
            edges = dict(ch)
            if terminal[n]:
                edges[eos] = 0
            for t in sorted(edges):
                edge_tok.append(t); edge_dst.append(edges[t])
            edge_off.append(len(edge_tok))
        self.vocab_size, self.eos_token_id, self.min_len = V, eos, int(min_len)
        self.sink = 0
        self.edge_off = np.asarray(edge_off, dtype=np.int32)
        self.edge_tok = np.asarray(edge_tok, dtype=np.int32)
        self.edge_dst = np.asarray(edge_dst, dtype=np.int32)
        self.roots = np.asarray(roots, dtype=np.int32)
        self.check(eos, min_new_tokens, V)

    n_nodes = property(lambda self: int(self.edge_off.shape[0]) - 1)
    n_edges = property(lambda self: int(self.edge_tok.shape[0]))
    n_sets = property(lambda self: int(self.roots.shape[0]))

    @property
    def key(self):
        """The content of the trie: what a cache of device copies is keyed by."""
        return (self.vocab_size, self.eos_token_id, self.edge_off.tobytes(), self.edge_tok.tobytes(), self.edge_dst.tobytes(), self.roots.tobytes())

    def check(self, eos_token_id, min_new_tokens: int = 0, vocab_size: Optional[int] = None):
        """The arguments of a generate() call against the trie: ValueError by name."""
        if isinstance(eos_token_id, (list, tuple)) and len(set(int(e) for e in eos_token_id)) == 1:
            eos_token_id = eos_token_id[0]
        if eos_token_id is None or isinstance(eos_token_id, (list, tuple)) or int(eos_token_id) != self.eos_token_id:
            raise ValueError(f"constrained generation: eos_token_id = {eos_token_id!r}, the trie was built with eos_token_id = {self.eos_token_id} "
                             "(one EOS id is required: an answer ends by emitting it)")
        if vocab_size is not None and int(vocab_size) != self.vocab_size:
            raise ValueError(f"constrained generation: the trie was built for vocab_size = {self.vocab_size}, the model has {int(vocab_size)}")
        if int(min_new_tokens or 0) > self.min_len:
            raise ValueError(f"constrained generation: min_new_tokens = {int(min_new_tokens)} exceeds the shortest allowed sequence ({self.min_len} "
                             "tokens): with the EOS edge suppressed at its end nothing would be allowed")

    def _walk(self, set_index: int, prefix_ids: Sequence[int]) -> int:
        """Node reached from the root of `set_index` along prefix_ids, -1 when the prefix leaves the trie."""
        n = int(self.roots[set_index])
        for t in prefix_ids:
            lo, hi = int(self.edge_off[n]), int(self.edge_off[n + 1])
            j = lo + int(np.searchsorted(self.edge_tok[lo:hi], int(t)))
            if j >= hi or int(self.edge_tok[j]) != int(t):
                return -1
            n = int(self.edge_dst[j])
        return n

    def allowed(self, set_index: int, prefix_ids: Sequence[int]) -> List[int]:
        """The host walker: the sorted ids allowed after `prefix_ids` (the ids generated so far) in set `set_index` - what a
        prefix_allowed_tokens_fn would return.  [] after a prefix that is no prefix of a member followed by EOS."""
        n = self._walk(set_index, prefix_ids)
        if n < 0:
            return []
        return [int(t) for t in self.edge_tok[int(self.edge_off[n]):int(self.edge_off[n + 1])]]

    def is_member(self, set_index: int, ids: Sequence[int]) -> bool:
        """ids (cut before EOS) is one of the sequences of the set."""
        n = self._walk(set_index, ids)
        return n >= 0 and self.eos_token_id in self.allowed(set_index, ids)

    @classmethod
    def from_strings(cls, tokenizer, answer_sets, vocab_size: Optional[int] = None, eos_token_id=None, min_new_tokens: int = 0):
        """Answer strings -> trie, every answer tokenised by the reference's rule and nothing else (dataset/AVQA.py:149):
        tokenizer.convert_tokens_to_ids(tokenizer.tokenize(s)).  answer_sets: a list of strings (one set) or a list of such lists."""
        answer_sets = list(answer_sets)
        if answer_sets and isinstance(answer_sets[0], str):
            answer_sets = [answer_sets]
        sets = [[tokenizer.convert_tokens_to_ids(tokenizer.tokenize(s)) for s in group] for group in answer_sets]
        if vocab_size is None:
            vocab_size = len(tokenizer)
        if eos_token_id is None:
            eos_token_id = getattr(tokenizer, "eos_token_id", None)
        return cls(sets, vocab_size, eos_token_id, min_new_tokens)


def as_trie(allowed_sequences, vocab_size: int, eos_token_id, min_new_tokens: int = 0) -> TokenTrie:
    """The `allowed_sequences` argument of generate(): a TokenTrie, one list of id sequences (one set for every row) or a list of such lists."""
    if isinstance(allowed_sequences, TokenTrie):
        allowed_sequences.check(eos_token_id, min_new_tokens, vocab_size)
        return allowed_sequences
    seqs = list(allowed_sequences)
    if not seqs:
        raise ValueError("allowed_sequences is empty")

    def is_id(x):
        return not hasattr(x, "__len__") or (hasattr(x, "dim") and x.dim() == 0)

    first = seqs[0]
    if hasattr(first, "tolist"):
        first = first.tolist()
    one_set = len(first) == 0 or is_id(first[0])               # [[1, 2], [3]]: elements of the first entry are ids, not sequences
    sets = [seqs] if one_set else seqs
    sets = [[(s.tolist() if hasattr(s, "tolist") else list(s)) for s in group] for group in sets]
    return TokenTrie(sets, vocab_size, eos_token_id, min_new_tokens)


def rows_of(trie: TokenTrie, allowed_set, n_rows: int, what: str = "allowed_set") -> List[int]:
    """One set index per row -> validated list; None = set 0 for every row (an error when the trie holds several sets)."""
    if allowed_set is None:
        if trie.n_sets > 1:
            raise ValueError(f"{what}: allowed_sequences holds {trie.n_sets} sets, so every row needs a set index ({what} is None)")
        return [0] * n_rows
    idx = [int(i) for i in (allowed_set.tolist() if hasattr(allowed_set, "tolist") else allowed_set)]
    if len(idx) != n_rows:
        raise ValueError(f"{what}: {len(idx)} set indices for {n_rows} rows")
    if any(not 0 <= i < trie.n_sets for i in idx):
        raise ValueError(f"{what}: a set index is outside [0, {trie.n_sets})")
    return idx
