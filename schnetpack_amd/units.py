"""Unit conversion for the two constructor arguments of ``ZBLRepulsionEnergy`` (``energy_unit``, ``position_unit``): a small stand-in
for ``schnetpack.units.convert_units`` (units.py:184-186), which resolves unit names through ``ase.units``.

``ase`` is not a dependency of this package, so the factors are derived here, from the CODATA-2014 constants, by the same chain of
definitions ``ase.units`` uses (eV and Angstrom are 1; Bohr and Hartree follow from the electron mass, the elementary charge, the
vacuum permittivity and hbar; kJ = 1000 / e; kcal = 4.184 kJ; mol = the Avogadro number).  The values have NOT been compared against
an installed ``ase``: none was available where this module was written and tested.  tests/test_zbl_reference.py pins them to the
published CODATA-2014 figures (Bohr radius 0.52917721067 A, Hartree 27.21138602 eV) instead.

Only the names the reference's configurations pass for those two arguments are known: ``Ha`` / ``Hartree``, ``eV``, ``kcal/mol``,
``kJ/mol``, ``Bohr``, ``Ang`` / ``Angstrom``, ``nm``.  Numbers are taken as they are (a factor in eV resp. Angstrom)."""
import math
from typing import Union

__all__ = ["convert_units", "KNOWN_UNITS"]

# CODATA 2014
_c = 299792458.0
_mu0 = 4.0e-7 * math.pi
_hplanck = 6.626070040e-34
_e = 1.6021766208e-19
_me = 9.10938356e-31
_Nav = 6.022140857e23

_eps0 = 1.0 / _mu0 / _c ** 2
_hbar = _hplanck / (2.0 * math.pi)

_kJ = 1000.0 / _e
_UNITS = {
    "eV": 1.0,
    "Ang": 1.0,
    "Angstrom": 1.0,
    "nm": 10.0,
    "Bohr": 4e10 * math.pi * _eps0 * _hbar ** 2 / _me / _e ** 2,
    "Hartree": _me * _e ** 3 / 16.0 / math.pi ** 2 / _eps0 ** 2 / _hbar ** 2,
    "kJ": _kJ,
    "kcal": 4.184 * _kJ,
    "mol": _Nav,
}
_UNITS["Ha"] = _UNITS["Hartree"]

KNOWN_UNITS = ["Ha", "Hartree", "eV", "kcal/mol", "kJ/mol", "Bohr", "Ang", "Angstrom", "nm"]


def _parse(unit: Union[str, float]) -> float:
    if not isinstance(unit, str):
        return float(unit)
    name = unit.replace(" ", "")
    if name not in KNOWN_UNITS:
        raise ValueError("unknown unit %r: schnetpack_amd.units knows %s (or pass the factor as a number)" % (unit, ", ".join(KNOWN_UNITS)))
    value = 1.0
    for k, part in enumerate(name.split("/")):
        value = value * _UNITS[part] if k == 0 else value / _UNITS[part]
    return value


def convert_units(src_unit: Union[str, float], tgt_unit: Union[str, float]) -> float:
    """Factor that converts a quantity given in ``src_unit`` into ``tgt_unit`` (units.py:184-186: parse(src) / parse(tgt))."""
    return _parse(src_unit) / _parse(tgt_unit)
