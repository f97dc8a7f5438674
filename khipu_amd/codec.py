"""Host-side key/value codecs for the state-root path (pure Python, no GPU).

These serialise what khipu hands to ``MerklePatriciaTrie.put`` as bytes, so
callers of the C-ABI (and the tests) can build inputs the same way the reference
does.  Reference files (under /root/reference/):

* RLP string / list framing: khipu-base/.../rlp/RLP.scala:116-169
* account body RLP[nonce, balance, stateRoot, codeHash]:
  khipu-eth/.../network/p2p/messages/PV63.scala:46-51 (AccountEnc),
  values via rlp.toRLPEncodable(DataWord) (rlp/package.scala:56-57) =
  DataWord.nonZeroLeadingBytes (DataWord.scala:175-188), zero -> empty string
* storage value = rlp.encode(toRLPEncodable(DataWord)) (trie/package.scala:28-32)
* EMPTY_TRIE_HASH / EMPTY_CODE_HASH: domain/Account.scala:13-17
"""

EMPTY_TRIE_HASH = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")
EMPTY_CODE_HASH = bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")
EMPTY_LIST_HASH = bytes.fromhex("1dcc4de8dec75d7aab85b567b6ccd41ad312451b948a7413f0a142fd40d49347")


def _len_prefix(n: int, offset: int) -> bytes:
    """RLP.encodeLength (RLP.scala:157-169)."""
    if n < 56:
        return bytes([n + offset])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([len(be) + offset + 55]) + be


def rlp_str(b: bytes) -> bytes:
    """RLPValue encoding (RLP.scala:141-150): one byte < 0x80 is its own encoding."""
    if len(b) == 1 and b[0] < 0x80:
        return bytes(b)
    return _len_prefix(len(b), 0x80) + bytes(b)


def rlp_list(*items: bytes) -> bytes:
    """RLPList of already-encoded items (RLP.scala:118-139)."""
    payload = b"".join(items)
    return _len_prefix(len(payload), 0xC0) + payload


def uint_bytes(v: int) -> bytes:
    """Minimal big-endian bytes; 0 -> b'' (DataWord.nonZeroLeadingBytes / isZero)."""
    if v < 0:
        raise ValueError("negative")
    return v.to_bytes((v.bit_length() + 7) // 8, "big") if v else b""


def account_rlp(nonce: int, balance: int, state_root: bytes = EMPTY_TRIE_HASH,
                code_hash: bytes = EMPTY_CODE_HASH) -> bytes:
    """Account body bytes, as Account.accountSerializer.toBytes (PV63.scala:46-51)."""
    return rlp_list(rlp_str(uint_bytes(nonce)), rlp_str(uint_bytes(balance)),
                    rlp_str(state_root), rlp_str(code_hash))


def storage_value_rlp(v: int) -> bytes:
    """Storage slot value bytes, as rlpDataWordSerializer.toBytes (trie/package.scala:28-32)."""
    return rlp_str(uint_bytes(v))


# ---- partial paths (snap's GetTrieNodes): a path is a sequence of nibbles, 0..64 of them
def nibbles_to_path32(nibbles) -> bytes:
    """A path as key bytes: packed big-endian, two nibbles a byte, zero-padded to 32 bytes (the
    form a stub record keeps its key prefix in)."""
    nib = list(nibbles) + [0] * (64 - len(nibbles))
    return bytes((nib[2 * i] << 4) | nib[2 * i + 1] for i in range(32))


def path32_to_nibbles(path32: bytes, n: int) -> list:
    """The first n nibbles of a packed 32-byte path."""
    return [(path32[i >> 1] >> 4) if i % 2 == 0 else (path32[i >> 1] & 0xF) for i in range(n)]


def path_to_compact(nibbles) -> bytes:
    """snap's wire form of a partial path: HexPrefix without the terminator flag (geth's
    hexToCompact of a path that does not end a key) -- 0x00 then the nibbles in pairs when their
    number is even, 0x1n then the rest when it is odd (1..33 bytes)."""
    nib = list(nibbles)
    if len(nib) > 64 or any(not 0 <= x < 16 for x in nib):
        raise ValueError("a path is at most 64 nibbles, each 0..15")
    if len(nib) % 2:
        head, rest = bytes([0x10 | nib[0]]), nib[1:]
    else:
        head, rest = b"\x00", nib
    return head + bytes((rest[i] << 4) | rest[i + 1] for i in range(0, len(rest), 2))


def path_from_compact(b: bytes) -> list:
    """The nibbles of a path in snap's wire form (path_to_compact's inverse)."""
    if not b or len(b) > 33:
        raise ValueError("a compact path is 1..33 bytes")
    flag = b[0] >> 4
    if flag > 1 or (flag == 0 and b[0] & 0xF):
        raise ValueError("not a partial path: bad HexPrefix flag")
    out = [b[0] & 0xF] if flag else []
    for x in b[1:]:
        out += [x >> 4, x & 0xF]
    return out
