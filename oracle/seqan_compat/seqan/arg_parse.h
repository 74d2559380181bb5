// seqan_compat/seqan/arg_parse.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
//
// ArgumentParser as main.cpp:94-199 builds it and Settings.cpp:74-123 reads it back.
//   * an option is given as `-short value` or `--long value`; a flag (an option declared
//     without an argument type) takes no value;
//   * parse() answers PARSE_OK, PARSE_ERROR, PARSE_HELP (-h / --help) or PARSE_VERSION
//     (--version); main.cpp:199 leaves with `res == PARSE_ERROR`, so help and version exit
//     with 0 and every error with 1 — the exit codes oracle/talc_ref_main.cpp has;
//   * errors: an unknown option, a missing value, a value that is no number where one is
//     declared, a value outside setMinValue / setMaxValue or not among setValidValues, a
//     required option that is not given, and a wrong number of positional arguments;
//   * getOptionValue / getArgumentValue by short or long name: the given value, else the
//     default, else the target is left as it is and false is returned; isSet() is true only
//     for an option given on the command line.
#pragma once
#include <cerrno>
#include <cstdlib>
#include <sstream>

#include "basic.h"

namespace seqan {

struct ArgParseArgument {
  enum ArgumentType { STRING, INTEGER, DOUBLE };
  ArgumentType type;
  std::string label;
  ArgParseArgument(ArgumentType t, const std::string& l = "") : type(t), label(l) {}
};

struct ArgParseOption {
  std::string shortName, longName, help, label;
  bool isFlag;
  ArgParseArgument::ArgumentType type;
  bool required = false, given = false, hasDefault = false, hasMin = false, hasMax = false;
  std::string value, defaultValue;
  double minValue = 0, maxValue = 0;
  std::vector<std::string> validValues;
  ArgParseOption(const std::string& s, const std::string& l, const std::string& h)
      : shortName(s), longName(l), help(h), isFlag(true), type(ArgParseArgument::STRING) {}
  ArgParseOption(const std::string& s, const std::string& l, const std::string& h, ArgParseArgument::ArgumentType t,
                 const std::string& lab = "")
      : shortName(s), longName(l), help(h), label(lab), isFlag(false), type(t) {}
};

class ArgumentParser {
 public:
  enum ParseResult { PARSE_OK, PARSE_ERROR, PARSE_HELP, PARSE_VERSION };
  std::string name, shortDescription, version, date;
  std::vector<ArgParseOption> options;
  std::vector<ArgParseArgument> arguments;
  std::vector<std::string> argumentValues;
  ArgumentParser(const std::string& n = "") : name(n) {}

  ArgParseOption* lookup(const std::string& n) {
    for (size_t i = 0; i < options.size(); ++i)
      if (options[i].shortName == n || options[i].longName == n) return &options[i];
    return nullptr;
  }
  ArgParseOption& get(const std::string& n) {
    ArgParseOption* o = lookup(n);
    if (!o) {
      std::fprintf(stderr, "seqan_compat: no option named %s\n", n.c_str());
      std::abort();
    }
    return *o;
  }
};

inline void setShortDescription(ArgumentParser& p, const std::string& s) { p.shortDescription = s; }
inline void setVersion(ArgumentParser& p, const std::string& s) { p.version = s; }
inline void setDate(ArgumentParser& p, const std::string& s) { p.date = s; }
inline void addArgument(ArgumentParser& p, const ArgParseArgument& a) { p.arguments.push_back(a); }
inline void addOption(ArgumentParser& p, const ArgParseOption& o) { p.options.push_back(o); }
inline void setRequired(ArgumentParser& p, const std::string& n, bool r = true) { p.get(n).required = r; }
template <typename T>
inline void setDefaultValue(ArgumentParser& p, const std::string& n, const T& v) {
  std::ostringstream os;
  os << v;
  p.get(n).defaultValue = os.str();
  p.get(n).hasDefault = true;
}
inline void setMinValue(ArgumentParser& p, const std::string& n, const std::string& v) {
  p.get(n).minValue = std::strtod(v.c_str(), nullptr);
  p.get(n).hasMin = true;
}
inline void setMaxValue(ArgumentParser& p, const std::string& n, const std::string& v) {
  p.get(n).maxValue = std::strtod(v.c_str(), nullptr);
  p.get(n).hasMax = true;
}
inline void setValidValues(ArgumentParser& p, const std::string& n, const std::string& values) {
  std::istringstream is(values);
  std::string v;
  while (is >> v) p.get(n).validValues.push_back(v);
}

inline bool compatNumber(const std::string& s, bool integer, double& out) {
  if (s.empty()) return false;
  char* end = nullptr;
  errno = 0;
  if (integer) out = (double)std::strtoll(s.c_str(), &end, 10);
  else out = std::strtod(s.c_str(), &end);
  return errno == 0 && end && *end == '\0';
}

inline ArgumentParser::ParseResult compatParseError(const ArgumentParser& p, const std::string& what) {
  std::cerr << p.name << ": " << what << "\n";
  return ArgumentParser::PARSE_ERROR;
}

inline ArgumentParser::ParseResult parse(ArgumentParser& p, int argc, const char* const* argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-h" || a == "--help") {
      std::cout << p.name << "\n" << p.shortDescription << "\n";
      for (size_t o = 0; o < p.options.size(); ++o)
        std::cout << "  -" << p.options[o].shortName << ", --" << p.options[o].longName << " " << p.options[o].label
                  << "\n      " << p.options[o].help << "\n";
      return ArgumentParser::PARSE_HELP;
    }
    if (a == "--version") {
      std::cout << p.name << " version: " << p.version << "\nLast update: " << p.date << "\n";
      return ArgumentParser::PARSE_VERSION;
    }
    if (a.size() > 1 && a[0] == '-') {
      ArgParseOption* o = nullptr;
      if (a[1] == '-') {
        for (size_t k = 0; k < p.options.size(); ++k)
          if (p.options[k].longName == a.substr(2)) o = &p.options[k];
      } else {
        for (size_t k = 0; k < p.options.size(); ++k)
          if (p.options[k].shortName == a.substr(1)) o = &p.options[k];
      }
      if (!o) return compatParseError(p, "illegal option -- " + a);
      o->given = true;
      if (o->isFlag) continue;
      if (i + 1 >= argc) return compatParseError(p, "option requires an argument -- " + a);
      o->value = argv[++i];
      if (o->type == ArgParseArgument::INTEGER || o->type == ArgParseArgument::DOUBLE) {
        double v = 0;
        if (!compatNumber(o->value, o->type != ArgParseArgument::DOUBLE, v))
          return compatParseError(p, "the given value '" + o->value + "' cannot be cast -- " + a);
        if ((o->hasMin && v < o->minValue) || (o->hasMax && v > o->maxValue))
          return compatParseError(p, "the given value '" + o->value + "' is not in the allowed interval -- " + a);
      }
      if (!o->validValues.empty() &&
          std::find(o->validValues.begin(), o->validValues.end(), o->value) == o->validValues.end())
        return compatParseError(p, "the given value '" + o->value + "' is not among the valid values -- " + a);
    } else {
      p.argumentValues.push_back(a);
    }
  }
  for (size_t k = 0; k < p.options.size(); ++k)
    if (p.options[k].required && !p.options[k].given)
      return compatParseError(p, "option -" + p.options[k].shortName + " is required");
  if (p.argumentValues.size() < p.arguments.size()) return compatParseError(p, "too few arguments");
  if (p.argumentValues.size() > p.arguments.size()) return compatParseError(p, "too many arguments");
  return ArgumentParser::PARSE_OK;
}

inline bool isSet(ArgumentParser& p, const std::string& n) { return p.get(n).given; }

inline void compatCast(std::string& out, const std::string& s) { out = s; }
template <typename T, typename S>
inline void compatCast(String<T, S>& out, const std::string& s) { out = s; }
inline void compatCast(double& out, const std::string& s) { out = std::strtod(s.c_str(), nullptr); }
template <typename T>
inline typename std::enable_if<std::is_integral<T>::value>::type compatCast(T& out, const std::string& s) {
  out = (T)std::strtoll(s.c_str(), nullptr, 10);
}

template <typename T>
inline bool getOptionValue(T& out, ArgumentParser& p, const std::string& n) {
  ArgParseOption& o = p.get(n);
  if (o.isFlag) return false;
  if (o.given) compatCast(out, o.value);
  else if (o.hasDefault) compatCast(out, o.defaultValue);
  else return false;
  return true;
}

template <typename T>
inline bool getArgumentValue(T& out, ArgumentParser& p, size_t i) {
  if (i >= p.argumentValues.size()) return false;
  compatCast(out, p.argumentValues[i]);
  return true;
}

}  // namespace seqan
