"""Maps for the wide table format (rl_map_register_wide; TEST INFRASTRUCTURE ONLY):
lakes past the packed table's 64 cells up to the cap of 1024, and the moat pair
that puts a 64-cell lake at state ids >= 256.

Checked with maps_model.predict_records (seed 0x5EED, 128 lanes, 128 steps,
max_steps 24, both env kinds, slippery 0 and 1): every L-map reaches every start,
goal, hole and truncation; the M1 and M2 records are identical under rel() except
plain FrozenLake's truncation observation, the literal state 0 in both (M1's cell 0
is an unreachable corner, so M1 state 0 <-> M2 state 0).
"""


def grid(nr, nc, starts, goals, hole):
    """'S' on the start indices, 'G' on the goal indices, 'H' where hole(r, c) holds
    unless the cell is a start or a goal, 'F' elsewhere; index = r * nc + c"""
    rows = []
    for r in range(nr):
        row = ""
        for c in range(nc):
            i = r * nc + c
            row += "S" if i in starts else "G" if i in goals else "H" if hole(r, c) else "F"
        rows.append(row)
    return rows


L65 = grid(5, 13, {64, 30}, {0}, lambda r, c: (r * 13 + c) % 7 == 3)        # first size past the packed table
L256 = grid(16, 16, {5, 130, 255}, {132}, lambda r, c: (r * 16 + c) % 11 == 4)
L300 = grid(3, 100, {299, 150}, {296}, lambda r, c: (r * 100 + c) % 9 == 5)  # cells past 255; not square
L1024 = grid(32, 32, {1023, 512}, {990}, lambda r, c: (r * 32 + c) % 13 == 6)  # the cap
LMAPS = {"L65": L65, "L256": L256, "L300": L300, "L1024": L1024}

# the moat pair: M1 (64 cells, rl_map_register) and M2 = a 20 x 20 lake of 'F' with M1
# copied to rows / columns 12..19 (400 cells, wide).  The moat of holes keeps every
# episode inside the copy.
M1 = ["HHHHHHHH", "HSFFFFFH", "HFFHFFFH", "HFFFGFFH", "HFHFFFFH", "HFFFFHFH", "HFFFFFSH", "HHHHHHHH"]
M2 = ["F" * 20] * 12 + ["F" * 12 + row for row in M1]


def rel(s):
    """M1 state -> M2 state"""
    return (12 + s // 8) * 20 + 12 + s % 8
