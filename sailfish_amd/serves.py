"""What each feature is served with: the table SERVES of csrc/slf_bind.h, row for row (tests/test_serves.py compares the
two).  A column is one field of the module descriptor; a row holds, per column, the mask of the field's values the
feature is served with (bit v: the value v; a yes / no field is served switched OFF only, or with ANY value).  A new
feature is one row here and one row there.

Names, order, per_node_only and masks are the library's.  The wording is the host's own on purpose: it names options as the
command line spells them and node types by class, carries notes the library has no use for (the elbm row's on
--regularized / --subgrid, which the library refuses one row earlier), and says what a field means where its name is the
ABI's (`says`)."""
from collections import namedtuple

from sailfish_amd import hipabi as h
from sailfish_amd import node_type as nt

# column -> its values as the user knows them (None: not worth listing); the node kinds by their classes
NAMES = {
    'lattice': ['D2Q9', 'D3Q19', 'D3Q15', 'D3Q27'],
    'simtype': ['single-fluid modules', 'the Shan-Chen models', 'the Shan-Chen models', 'the free-energy model', 'the ternary Shan-Chen model'],
    'model': ['--model=bgk', '--model=mrt', '--model=elbm'],
    'entropic_equilibrium': [None, '--entropic_equilibrium'], 'regularized': [None, '--regularized'], 'subgrid': [None, '--subgrid'],
    'incompressible': ['the compressible density model', '--incompressible', '--minimize_roundoff'],
    'node_addressing': ['--node_addressing=direct', '--node_addressing=indirect'],
    'has_force': [None, 'body forces'], 'accel_field': [None, 'accel_field'], 'force_implementation': [None, '--force_implementation=edm'],
    'type_kind': ['fluid'] + [None] * 16,
}
COLUMNS = tuple(NAMES)
for _cls, _kind in nt.HIP_KIND.items():
    if not _cls.__name__.startswith('_'):
        NAMES['type_kind'][_kind] = _cls.__name__


def bits(*values):
    """The mask of these values; bit 31 stands for every value without a bit of its own."""
    return sum(1 << (v if 0 <= v < 31 else 31) for v in values)


ANY, OFF = 0xFFFFFFFF, bits(0)
NO_EDM, NO_ELBM, NO_ROUNDOFF = ANY & ~bits(h.SLF_FORCE_EDM), ANY & ~bits(h.SLF_ELBM), ANY & ~bits(h.SLF_DENSITY_ROUNDOFF)
LBM, BGK, DIRECT = bits(h.SLF_SIM_LBM), bits(h.SLF_BGK), bits(h.SLF_ADDR_DIRECT)
COMPRESSIBLE, INCOMPRESSIBLE = bits(h.SLF_DENSITY_COMPRESSIBLE), bits(h.SLF_DENSITY_INCOMPRESSIBLE)
KINDS_PLAIN = bits(h.SLF_NK_FLUID, h.SLF_NK_GHOST, h.SLF_NK_UNUSED, h.SLF_NK_PROPAGATION_ONLY, h.SLF_NK_FULL_BB)
HALF_BB, SLIP, TMS = bits(h.SLF_NK_HALF_BB), bits(h.SLF_NK_SLIP), bits(h.SLF_NK_WALL_TMS)
EQUILIBRIUM = bits(h.SLF_NK_EQUILIBRIUM_DENSITY, h.SLF_NK_EQUILIBRIUM_VELOCITY)

# name, has, per_node_only, serves: the C row's.  notes: a reason worth telling, by column.  says: how messages call the
# feature, where not by its name.  columns: the columns the host applies (None: all of them) -- the rest is refused from the
# configuration before a descriptor exists (fill_module_desc, LBFluidSim.density_model), or by the library alone
Row = namedtuple('Row', 'name has per_node_only serves notes says columns', defaults=({}, None, None))
LAT = (ANY, LBM, BGK, OFF, OFF, OFF, NO_ROUNDOFF, DIRECT, ANY, ANY, ANY, KINDS_PLAIN | HALF_BB)
NOT_ENTROPIC = [c for c in COLUMNS if c != 'entropic_equilibrium']      # (LBFluidSim.check_module_desc's, for every lattice)
PREAMBLE = '--regularized / --subgrid belong to the BGK relaxation preamble, which the entropic collision never runs'
ROWS = (
    # masks: lattice, simtype, model, entropic, regularized, subgrid, density, addressing, force, accel_field, edm, kinds
    Row('shallow water', lambda kw: bool(kw.get('equilibrium')), True,
        (bits(h.SLF_D2Q9), LBM, BGK, OFF, OFF, OFF, COMPRESSIBLE, DIRECT, ANY, ANY, ANY, KINDS_PLAIN | HALF_BB | SLIP),
        {'incompressible': 'the density is the water depth',
         'type_kind': 'the node types that carry a density or a velocity assume the pressure rho / 3'}),
    Row('accel_field', lambda kw: bool(kw.get('accel_field')), True,
        (bits(h.SLF_D2Q9, h.SLF_D3Q19), LBM, NO_ELBM, ANY, OFF, OFF, NO_ROUNDOFF, DIRECT, ANY, ANY, ANY, ANY & ~TMS),
        {'lattice': 'the sweep of D3Q15 / D3Q27 takes a constant acceleration', 'model': 'the entropic collision takes no body force'},
        says='body forces that depend on position (accel_field)'),
    Row('D3Q15', lambda kw: kw.get('lattice') == h.SLF_D3Q15, True, LAT, columns=NOT_ENTROPIC),
    Row('D3Q27', lambda kw: kw.get('lattice') == h.SLF_D3Q27, True, LAT, columns=NOT_ENTROPIC),
    Row('regularized / subgrid', lambda kw: bool(kw.get('regularized') or kw.get('subgrid')), True,
        (ANY, LBM, BGK, ANY, ANY, ANY, NO_ROUNDOFF, ANY, ANY, ANY, NO_EDM, ANY), columns=()),
    Row('NTWallTMS', lambda kw: h.SLF_NK_WALL_TMS in kw.get('type_kind', []), True, (ANY, LBM) + (ANY,) * 10),
    Row('elbm', lambda kw: kw.get('model') == h.SLF_ELBM, True, (ANY, LBM, ANY, ANY, OFF, OFF, NO_ROUNDOFF, ANY, OFF, ANY, ANY, ANY),
        {'incompressible': 'it stores f_i - w_i, the entropy needs the populations themselves', 'regularized': PREAMBLE, 'subgrid': PREAMBLE}),
    Row('minimize_roundoff', lambda kw: kw.get('incompressible') == h.SLF_DENSITY_ROUNDOFF, True,
        (ANY, LBM, BGK) + (ANY,) * 8 + (KINDS_PLAIN | HALF_BB | TMS | EQUILIBRIUM,), columns=('type_kind',)),
    Row('Shan-Chen', lambda kw: kw.get('simtype') in (h.SLF_SIM_SHAN_CHEN_BINARY, h.SLF_SIM_SHAN_CHEN_SINGLE), False,
        (ANY, ANY, BGK) + (ANY,) * 8 + (KINDS_PLAIN,), columns=()),
    Row('free energy', lambda kw: kw.get('simtype') == h.SLF_SIM_FREE_ENERGY, False,
        (ANY, ANY, BGK, ANY, ANY, ANY, COMPRESSIBLE, DIRECT, OFF, ANY, ANY, KINDS_PLAIN),
        {'model': 'the FE-MRT collision, relaxation.mako:15-54', 'has_force': 'free_energy_external_force, use_force_for_equilibrium'},
        columns=('type_kind',)),
    Row('ternary Shan-Chen', lambda kw: kw.get('simtype') == h.SLF_SIM_SHAN_CHEN_TERNARY, False,
        (ANY, ANY, BGK, ANY, ANY, ANY, COMPRESSIBLE, DIRECT, ANY, ANY, ANY, KINDS_PLAIN), columns=('type_kind',)),
)
BY_NAME = dict((r.name, r) for r in ROWS)


def check(kw, names=None, always=False, columns=None):
    """Raises NotImplementedError for the first conflict of the descriptor fields `kw` with the rows that apply to it:
    '<feature>: <offender> is not served (<note>); <what the row serves> only', every offending node type class by name.
    `names`: these rows only; `always`: whether or not `kw` says it has the feature; `columns`: instead of the rows' own."""
    for row in ROWS if names is None else [BY_NAME[n] for n in names]:
        for column, mask in zip(COLUMNS, row.serves) if always or row.has(kw) else ():
            values = kw.get('type_kind', []) if column == 'type_kind' else [int(kw.get(column) or 0)]
            bad = [v for v in values if not mask & bits(v)]
            if not bad or column not in (columns or (COLUMNS if row.columns is None else row.columns)):
                continue
            if column == 'type_kind':
                who = sorted(cls.__name__ for cls, kind in nt.HIP_KIND.items() if kind in bad)
            else:
                who = [NAMES[column][v] for v in bad if 0 <= v < len(NAMES[column])]
            who = [w for w in who if w] or ['%s = %s' % (column, bad)]
            text = '%s: %s %s not served' % (row.says or row.name, ' / '.join(who), 'are' if len(who) > 1 or who[0].endswith('s') else 'is')
            if column in row.notes:
                text += ' (%s)' % row.notes[column]
            served = [name for v, name in enumerate(NAMES[column]) if name and mask & bits(v)]
            if 0 < len(served) <= 6:         # (a longer list says little more than the offender did)
                text += '; ' + ' and '.join([', '.join(served[:-1])] * (len(served) > 1) + served[-1:])
                text += ' nodes only' if column == 'type_kind' else ' only'
            raise NotImplementedError(text)


def config_fields(config, **fields):
    """The descriptor fields that the command line alone decides, for refusals before anything is built."""
    model = {'mrt': h.SLF_MRT, 'elbm': h.SLF_ELBM}.get(getattr(config, 'model', 'bgk'), h.SLF_BGK)
    density = h.SLF_DENSITY_ROUNDOFF if getattr(config, 'minimize_roundoff', False) else int(bool(getattr(config, 'incompressible', False)))
    return dict(fields, model=model, incompressible=density, regularized=int(bool(getattr(config, 'regularized', False))),
                subgrid=int(getattr(config, 'subgrid', 'none') not in ('none', None, '')),
                node_addressing=int(getattr(config, 'node_addressing', 'direct') != 'direct'))
